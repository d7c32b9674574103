"""rb_dev_swap in place (rb_k_swap_inplace) against the out-of-place kernel (rb_k_swap) on a config-3-shaped batch where it lies in HBM.

The batch is bench.py's headline workload (--records synthetic records of 1000-9000 ops, seed 0x5EED0003; about half of the records on
'-', the strands of rustybam_amd/workload.py).  Both calls are bracketed by HIP events on the engine's stream, alternating, warmed; the
median of --reps calls each.  Both kernels read every op once and write it once: 8 B per op.  One JSON line: both times, their spread, the
fraction of 8 TB/s.  No oracle: parity is the business of tests/test_gpu_swap_inplace.py (the in-place calls here run an even number of
times, so the batch ends as it began -- checked against the out-of-place result).

  python tools/bench_swap.py [--records 1000000] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import rustybam_amd
    from rustybam_amd import workload as wl
    from devutil import _i64
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    n, seed = a.records, wl.SEED_CONFIG3
    off = wl.op_offsets(wl.n_ops(seed, 0, n))
    total_ops = int(off[-1])
    d_off = _i64(torch, dev, off)
    d_ops = torch.empty(total_ops + 64, dtype=torch.int32, device=dev)
    d_out = torch.empty(total_ops + 64, dtype=torch.int32, device=dev)
    eng.dev_synth_fill_ops(seed, 0, n, d_off.data_ptr(), d_ops.data_ptr())
    z = np.zeros(n, np.uint64)
    strand = wl.headers(seed, 0, z, z)[4]
    d_strand = torch.from_numpy(np.ascontiguousarray(strand)).to(dev)
    v = eng.batch_view(n, total_ops, d_ops.data_ptr(), d_off.data_ptr(), 0, 0, 0, 0, d_strand.data_ptr(), 0)
    torch.cuda.synchronize()

    def timed(out_ptr):
        e0, e1 = ev(), ev()
        e0.record()
        rc = eng.dev_swap(v, out_ptr)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        return e0.elapsed_time(e1)

    ms_in, ms_out = [], []
    for i in range(4 + 2 * (a.reps // 2)):  # alternating; an even number of in-place calls
        t_out, t_in = timed(d_out.data_ptr()), timed(d_ops.data_ptr())
        if i >= 4:
            ms_out.append(t_out), ms_in.append(t_in)
    # the batch is as it began: one more out-of-place call, one in-place call, and the two arrays must be equal
    timed(d_out.data_ptr()), timed(d_ops.data_ptr())
    same = bool(torch.equal(d_ops[:total_ops], d_out[:total_ops]))
    timed(d_ops.data_ptr())
    moved = 8 * total_ops
    r = lambda x: round(float(x), 4)  # noqa: E731
    print(json.dumps({
        "what": "rb_dev_swap on a config-3-shaped batch (HIP events, warmed, alternating, median)", "records": n, "ops": total_ops,
        "minus_fraction": r((strand == ord("-")).mean()), "reps": len(ms_in),
        "in_place_ms": r(np.median(ms_in)), "in_place_ms_min": r(min(ms_in)), "in_place_ms_max": r(max(ms_in)),
        "out_of_place_ms": r(np.median(ms_out)), "out_of_place_ms_min": r(min(ms_out)), "out_of_place_ms_max": r(max(ms_out)),
        "algorithmic_bytes": moved, "in_place_fraction_of_8TBps": r(moved / (np.median(ms_in) * 1e-3) / PEAK),
        "out_of_place_fraction_of_8TBps": r(moved / (np.median(ms_out) * 1e-3) / PEAK), "in_place_equals_out_of_place": same}))
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
