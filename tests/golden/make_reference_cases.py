#!/usr/bin/env python3
"""Record the REFERENCE coder's results (oracle/_ref/libfecpp_ref.so, see make_golden.py) for the seeded
differential cases of tests/reference_cases.py.  Run where the reference is compiled:

    make -C oracle && python tests/golden/make_reference_cases.py

Output (committed; data only -- case parameters and digests of the reference's outputs):
  reference_cases.json
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import reference_cases  # noqa: E402
from oracle import RefCoder  # noqa: E402


def main() -> None:
    rec = reference_cases.record(RefCoder())
    with open(os.path.join(HERE, "reference_cases.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
