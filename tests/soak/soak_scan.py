"""Soak of the record scan's row form (rb_k_scan_rows): the generator of tests/scan_util.py over seeds -- every boundary length at every
start phase, one-defect records, hostile neighbours, wavefronts of mixed fate, the routing boundary, magnitudes -- each batch against
the per-base oracle and the flag reference, route asserted, plus one batch of random short records a seed.

    python3 tests/soak/soak_scan.py [seeds] [first seed]
"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: F401 (before the library: one copy of the HIP runtime a process, tests/conftest.py)
import rustybam_amd
from oracle import pyoracle as oracle
import scan_util as su

oracle.build()
eng = rustybam_amd.Engine(0)
n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
records = took = listed = 0
for seed in range(seed0, seed0 + n_seeds):
    gen = su.batches(seed)
    gen["random_short"] = su.random_short_batch(np.random.default_rng(seed), int(np.random.default_rng(seed).integers(64, 20000)))
    for name, b in gen.items():
        su.check_scan(eng, oracle, b, f"seed {seed}: {name}", "wave" if name in su.WAVE_BATCHES else "rows")
        t, l = eng.scan_route()
        records, took, listed = records + len(b["op_off"]) - 1, took + t, listed + l
print(f"soak_scan ok: {n_seeds} seeds from {seed0}, {records} records, {took} scanned by the row form, {listed} listed by it")
