"""rb_dev_largest (liftover --largest, main.rs:200-208) on the hit rows of one config-3 liftover step, where they lie in HBM.

The batch is bench.py's headline workload (BASELINE.json configs[2]: --records synthetic records of 1000-9000 ops, seed 0x5EED0003, placed
uniformly on a chr1-sized target, 3000 sliding windows of 100 kb): built on the device, lifted once with the fused scan, and the rows of
that step -- about 12.6 per record -- are what rb_dev_largest reduces.  Every window is a key of its own; records that lie inside a
window take the key of the empty id, so the key space is n_win + 1.  The call is bracketed by HIP events on the engine's stream with its
outputs and scratch allocated before: warmed, the median of --reps calls.  One JSON line: kernel_ms, the bytes the call has to move
(32 B per row per pass over the rows, 16 B per key), the fraction of 8 TB/s, and the ratio to the clip step it runs behind (timed here
the same way, three launches).  No oracle: parity is the business of tests/test_gpu_largest.py.

  python tools/bench_largest.py [--records 1000000] [--windows 3000] [--reps 30]
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
    ap.add_argument("--windows", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import rustybam_amd
    from rustybam_amd import workload as wl
    from devutil import DevBatch, _i64
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    # ---- the batch: ops by the library's generator, headers from the spans the record scan returns (as bench.py does) ----
    n, seed = a.records, wl.SEED_CONFIG3
    off = wl.op_offsets(wl.n_ops(seed, 0, n))
    total_ops = int(off[-1])
    d_off = _i64(torch, dev, off)
    d_ops = torch.empty(total_ops + 64, dtype=torch.int32, device=dev)
    eng.dev_synth_fill_ops(seed, 0, n, d_off.data_ptr(), d_ops.data_ptr())
    zeros = torch.zeros(n, dtype=torch.int64, device=dev)
    d_red = torch.empty(n * 72, dtype=torch.uint8, device=dev)
    v0 = eng.batch_view(n, total_ops, d_ops.data_ptr(), d_off.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), zeros.data_ptr(),
                        torch.full((n,), ord("+"), dtype=torch.uint8, device=dev).data_ptr(), torch.zeros(n, dtype=torch.int32, device=dev).data_ptr())
    torch.cuda.synchronize()
    eng.dev_scan_records(v0, d_red.data_ptr(), 0)
    torch.cuda.synchronize()
    red = d_red.cpu().numpy().view(rustybam_amd.REDUCE_DT)
    del d_red
    t_st, t_en, q_st, q_en, strand = wl.headers(seed, 0, red["t_bases"], red["q_bases"])
    D = DevBatch.from_device(torch, eng, dev, d_ops, total_ops, off, [_i64(torch, dev, x) for x in (t_st, t_en, q_st, q_en)],
                             torch.from_numpy(strand).to(dev))
    w = wl.sliding_windows(a.windows)
    POL = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN
    rows, out, cnt = D.run(w, policy=POL, rows_cap=14 * n + 1024)
    n_rows = int(cnt["n_hits"])
    rows_buf, out_buf, ws_ = D.last  # (uint8 [(rows_cap + 1) * 64], int32 [out_cap + 64], the workspace of that rows_cap)
    plan = eng.plan_create(D.op_off_host, D.contig_host, *w)
    step_ms = []
    for _ in range(3):  # the clip step the call runs behind, on the buffers the sizing loop ended with
        e0, e1 = ev(), ev()
        e0.record()
        eng.dev_liftover(plan, D.view, D.d_norm.data_ptr(), POL, ws_.data_ptr(), rows_buf.data_ptr(), rows_buf.numel() // 64 - 1, out_buf.data_ptr(),
                         out_buf.numel() - 64, D.d_cnt.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        step_ms.append(e0.elapsed_time(e1))
    eng.plan_destroy(plan)

    # ---- keys: window i has key i + 1, the empty id (records inside a window) key 0 ----
    n_keys = a.windows + 1
    d_wk = torch.arange(1, n_keys, dtype=torch.int32, device=dev)
    d_rk = torch.zeros(n, dtype=torch.int32, device=dev)
    d_sel = torch.zeros(n_keys, dtype=torch.int64, device=dev)
    d_out = torch.zeros(2, dtype=torch.int64, device=dev)
    d_scr = torch.empty(eng.largest_scratch_bytes(n_keys), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ms = []
    for i in range(5 + a.reps):
        e0, e1 = ev(), ev()
        e0.record()
        eng.dev_largest(rows.data_ptr(), n_rows, d_wk.data_ptr(), d_rk.data_ptr(), n_keys, d_sel.data_ptr(), d_out.data_ptr(), d_scr.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    o = d_out.cpu().numpy()
    h = rows.cpu().numpy().view(np.uint8).reshape(-1).view(rustybam_amd.HIT_DT)
    inside = int(((h["flags"] & rustybam_amd.HIT_INSIDE) != 0).sum())
    med, step = float(np.median(ms)), float(np.median(step_ms))
    moved = 2 * 32 * n_rows + 16 * n_keys
    print(json.dumps({
        "what": "rb_dev_largest on the hit rows of one config-3 liftover step (HIP events, warmed, median)",
        "records": n, "windows": a.windows, "rows": n_rows, "rows_inside": inside, "n_keys": n_keys, "n_sel": int(o[0]), "n_bad": int(o[1]),
        "reps": len(ms), "kernel_ms": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
        "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4),
        "clip_step_ms": round(step, 3), "ratio_to_clip_step": round(med / step, 4)}))
    eng.close()


if __name__ == "__main__":
    main()
