"""bench.py's single-GPU line as the driver reads it: one JSON line on stdout, the roofline with every
same-run ceiling -- the linear read, calib_mix at several occupancies, the product kernel's own arithmetic-free build
(tools/libkfec_arithfree.so) at several occupancies -- and the verification flag, for an encode+decode config and the
decode-only one.  Small batches: this checks the measurement path, not the numbers."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("config", ["20:3", "10:3dec"])
def test_bench_line_carries_the_same_run_ceilings(config):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, "bench.py", "--config", config, "--groups", "16384", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu"], cwd=ROOT, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["verified_bit_exact"] and d["n_gpus"] == 1 and d["value"] > 0
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and 0 < roof["frac"] < 1.2 and roof["read_ceiling"] > 0
    # the arithmetic-free build of the product kernel ran, at its own occupancy and capped
    af = roof["arithfree_ms_by_occupancy"]
    assert roof["arithfree_ms"] and set(af) >= {"own", "4w", "3w", "2w"} and all(v > 0 for v in af.values())
    assert set(roof["mix_calib_GBps_by_occupancy"]) >= {"own", "4w", "3w", "2w"}
    # the mix ceiling is the fastest candidate, and says which one it was
    best_af = roof["algorithmic_bytes_per_launch"] / (min(af.values()) * 1e-3) / 1e9
    best = max(best_af, max(roof["mix_calib_GBps_by_occupancy"].values()))
    assert abs(roof["mix_ceiling"] - best) <= 0.002 * best
    assert roof["mix_ceiling_kind"] in ("arithfree", "calib_mix")
    assert roof["frac_of_mix_ceiling"] == pytest.approx(roof["achieved"] / roof["mix_ceiling"], rel=2e-3)


@pytest.mark.parametrize("config", ["20:3", "10:3dec"])
def test_plain_run_times_its_steps_and_dumps_what_they_computed(config, tmp_path, oracle):
    """Without --full the line carries the headline (value, ms_per_step over exactly --steps steps) and nothing that
    takes a run of its own; --dump-outputs writes float32 arrays of a sample of groups fixed by the arguments, which
    equal the oracle's parity / recovered shards / ids / status for the bench's seeded inputs.  2050 groups: more
    than the dump budget holds for 20:3 (a sample), not a multiple of any tile."""
    import numpy as np
    import torch

    import bench
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    G = 2050
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", config, "--groups", str(G), "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    K, N, B, _, pool, erase, mode, do_enc, _ = bench.CONFIGS[config]
    R = N - K
    assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["decode_ms"] > 0
    assert d["value"] == pytest.approx(K * B * G / (d["ms_per_step"] * 1e-3) / 2**30, rel=1e-2)
    assert d["full"] is False and d["roofline"] is None and d["cpu_baseline"] is None
    assert d["verified_bit_exact"] is None and d["recovered_shards_per_step"] is None

    names = {"groups", "recovered", "recovered_ids", "status"} | ({"parity"} if do_enc else set())
    assert {p.name for p in tmp_path.iterdir()} == {n + ".npy" for n in names}
    got = {n: np.load(tmp_path / (n + ".npy"), allow_pickle=False) for n in names}
    assert all(a.dtype == (np.float64 if n == "groups" else np.float32) for n, a in got.items())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    sel = bench.dump_groups(G, R, B)
    assert len(sel) == len(set(sel.tolist())) == bench.DUMP_BUDGET // (4 * (2 * R * B + R + 1) + 8) < G
    np.testing.assert_array_equal(got["groups"], sel)

    data = oracle.synth(bench.SEED, N, B, 0, G, 0, K)
    par = oracle.encode_batch(K, N, data, B)
    masks = oracle.erasure_masks(bench.SEED, G, N, pool, erase, random_max=erase if mode == 1 else None)
    exp_out, exp_idx, exp_st = oracle.decode_batch(K, N, data, par, masks, B)
    exp_out[exp_idx == 0xFF] = 0
    if do_enc:
        np.testing.assert_array_equal(got["parity"], par[sel])
    np.testing.assert_array_equal(got["recovered_ids"], exp_idx[sel])
    np.testing.assert_array_equal(got["status"], exp_st[sel])
    np.testing.assert_array_equal(got["recovered"], exp_out[sel])
    assert (exp_idx[sel] != 0xFF).any()


@pytest.mark.parametrize("K,N", [(20, 23), (8, 12), (40, 60), (200, 255)])
def test_arithfree_build_has_no_gf_arithmetic(K, N):
    """The ceiling build must not carry any of the product's GF arithmetic (a paired or burst MAC branch that forgot
    the XOR-only knob would make the 'ceiling' the product itself): its every parity row is the plain XOR of the
    group's data shards."""
    import ctypes
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    path = os.path.join(ROOT, "tools", "libkfec_arithfree.so")
    assert os.path.exists(path), "build it first: kcptube_amd.build.build_tools()"
    lib = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.kfec_create.argtypes = [sz, sz, ctypes.POINTER(vp)]
    lib.kfec_destroy.argtypes = [vp]
    lib.kfec_encode_batch.argtypes = [vp, sz, sz, sz, vp, vp, vp]
    ctx = vp()
    assert lib.kfec_create(K, N, ctypes.byref(ctx)) == 0
    try:
        G, B = 96, 1440
        gen = torch.Generator().manual_seed(K * 1000 + N)
        data = torch.randint(0, 256, (G, K, B), dtype=torch.uint8, generator=gen).cuda()
        parity = torch.zeros((G, N - K, B), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream()
        assert lib.kfec_encode_batch(ctx, G, B, B, data.data_ptr(), parity.data_ptr(), vp(st.cuda_stream)) == 0
        torch.cuda.synchronize()
        x = data[:, 0].clone()
        for j in range(1, K):
            x ^= data[:, j]
        assert torch.equal(parity, x.unsqueeze(1).expand(G, N - K, B))
    finally:
        lib.kfec_destroy(ctx)


def test_bench_line_200_55_is_priced_against_the_paired_mac_bound():
    """fec=200:55 is VALU-bound: the line's roofline is byte-MACs/s against the issue bound of the paired perm MAC
    the 8-row kernels use (6 v_perm_b32 + 3 v_bitop3_b32 per 8 byte-MACs), with the single-shard form's bound kept
    beside it; the arithmetic-free build of the encode, the HBM side's ceiling, must be far faster than the product."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, "bench.py", "--config", "200:55", "--groups", "16384", "--steps", "2", "--full",
                        "--warmup", "1", "--no-cpu"], cwd=ROOT, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    roof = d["roofline"]
    assert d["verified_bit_exact"] and roof["bound"] == "valu" and roof["unit"] == "byte-MAC/s"
    assert roof["issue_bound_single"] < roof["peak"]  # the paired form issues fewer instructions per byte-MAC
    assert 0 < roof["frac"] < 1 and roof["frac"] < roof["frac_of_single_bound"]
    assert roof["arithfree_ms"] < 0.5 * d["encode_ms"]
