"""The seeded differential cases of tests/test_oracle.py against the reference coder, in a form that can be
recorded: record(coder) runs them through any coder with the fec_code interface (oracle.Oracle, oracle.RefCoder)
and returns plain data -- per-case SHA-256 digests of parity and decode results, and recovered ids.
tests/golden/make_reference_cases.py stores record(RefCoder()) as tests/golden/reference_cases.json, so the tests
hold the oracle to the reference's own results where the reference cannot be compiled."""
from __future__ import annotations

import hashlib

import numpy as np


def _sha(*parts: bytes) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(len(p).to_bytes(8, "little"))
        h.update(p)
    return h.hexdigest()


def _decoded(out: dict) -> list[bytes]:
    """a decode result {id: block} as a flat list: id, block, id, block ... in id order"""
    return [x for i in sorted(out) for x in (int(i).to_bytes(2, "little"), out[i])]


def randomized(coder) -> list[dict]:
    """200 random (K, N, B): encode, then decode from K-1..N shares, one of them corrupted in 30% of the cases."""
    rng = np.random.default_rng(2024)
    rows = []
    for _ in range(200):
        K = int(rng.integers(1, 48))
        N = int(min(256, K + rng.integers(0, 12)))
        B = int(rng.integers(1, 100))
        data = rng.integers(0, 256, K * B, dtype=np.uint8).tobytes()
        par = coder.encode(K, N, data, B)
        shards = {i: data[i * B:(i + 1) * B] for i in range(K)}
        for r, p in enumerate(par):
            shards[K + r] = p
        keep = sorted(rng.choice(N, int(rng.integers(max(K - 1, 0), N + 1)), replace=False).tolist())
        sub = {s: shards[s] for s in keep}
        if keep and rng.random() < 0.3:
            k = keep[int(rng.integers(len(keep)))]
            sub[k] = bytes(x ^ 0x5A for x in sub[k])
        out = coder.decode(K, N, sub, B)
        rows.append({"K": K, "N": N, "B": B, "keep": keep, "parity_sha": _sha(*par), "decode_ids": sorted(out),
                     "decode_sha": _sha(*_decoded(out))})
    return rows


def matrices(coder) -> list[dict]:
    """the encoding matrix of every K <= 32 at four N"""
    return [{"K": K, "N": N, "sha": _sha(np.ascontiguousarray(coder.enc_matrix(K, N)).tobytes())}
            for K in range(1, 33) for N in (K, K + 1, K + 3, min(256, K + 40))]


def share_size_zero(coder) -> list[dict]:
    """decode(shares, 0) of empty shares: which ids come back (each as an empty block)"""
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(60):
        K = int(rng.integers(1, 30))
        N = int(min(256, K + rng.integers(0, 8)))
        keep = sorted(rng.choice(N + 2, int(rng.integers(max(K - 1, 0), N + 1)), replace=False).tolist())
        out = coder.decode(K, N, {s: b"" for s in keep}, 0)
        rows.append({"K": K, "N": N, "keep": keep, "ids": sorted(int(i) for i in out),
                     "all_empty": all(v == b"" for v in out.values())})
    return rows


def record(coder) -> dict:
    return {"randomized": randomized(coder), "matrices": matrices(coder), "share_size_zero": share_size_zero(coder)}
