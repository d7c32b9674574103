"""rb_dev_stats_rows (k_hitstats.hip) alone, on the hit rows and clips of one clip step where they lie in HBM.

  config 3   bench.py's headline workload (--records synthetic records of 1000-9000 ops, seed 0x5EED0003, 3000 sliding windows of 100 kb):
             lifted once with the fused scan, plain (the clips are ops in out_ops) and with RB_LIFT_DESCRIPTORS (4-word descriptors into
             the batch; what the text route uses)
  config 4   --records4 records of 300-700 ops (SURVEY 8d config 4's shape), broken with --max-size 100: rows of about 100 ops

The call is bracketed by HIP events on the engine's stream with its output allocated before: warmed, the median of --reps calls.  One JSON
line per case: kernel_ms, the bytes the call has to move (64 B per row read, 72 B per row written, 4 B per clip op, 16 B per descriptor),
the fraction of 8 TB/s, and the ratio to the clip step it runs behind (timed here the same way, three launches).  No oracle: parity is the
business of tests/test_gpu_hitstats.py; here only the self-check is looked at (every stats row of an OK hit row has status 0).

  python tools/bench_hitstats.py [--records 1000000] [--windows 3000] [--records4 2000000] [--reps 20]
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
    ap.add_argument("--records4", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import rustybam_amd
    from rustybam_amd import workload as wl
    from devutil import DevBatch, _i64, config4_resident
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def measure(what, D, windows, policy, max_size, rows_cap):
        rows, out, cnt = D.run(windows, policy=policy, max_size=max_size, rows_cap=rows_cap)
        n_rows = int(cnt["n_hits"])
        rows_buf, out_buf, ws_ = D.last
        plan = eng.plan_create(D.op_off_host, D.contig_host, *(windows if windows is not None else (None, None, None)))
        step_ms = []
        for _ in range(3):  # the clip step the call runs behind, on the buffers the sizing loop ended with
            e0, e1 = ev(), ev()
            e0.record()
            if max_size is None:
                eng.dev_liftover(plan, D.view, D.d_norm.data_ptr(), policy, ws_.data_ptr(), rows_buf.data_ptr(), rows_buf.numel() // 64 - 1, out_buf.data_ptr(),
                                 out_buf.numel() - 64, D.d_cnt.data_ptr())
            else:
                eng.dev_break(plan, D.view, D.d_norm.data_ptr(), max_size, policy, ws_.data_ptr(), rows_buf.data_ptr(), rows_buf.numel() // 64 - 1,
                              out_buf.data_ptr(), out_buf.numel() - 64, D.d_cnt.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            step_ms.append(e0.elapsed_time(e1))
        eng.plan_destroy(plan)
        d_stats = torch.empty((n_rows + 1) * 72, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = ev(), ev()
            e0.record()
            eng.dev_stats_rows(D.view, rows.data_ptr(), n_rows, out.data_ptr(), d_stats.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        ok = (rows[:, 2] & 0xFFFF) == 0
        is_desc = ((rows[:, 2] >> 16) & rustybam_amd.HIT_DESCRIPTOR) != 0
        clip_ops = int(rows[:, 3].to(torch.int64)[ok].sum().item())
        n_ok, n_desc = int(ok.sum().item()), int((ok & is_desc).sum().item())
        n_long = int((ok & (rows[:, 3] > 4096)).sum().item())
        st = d_stats[: n_rows * 72].view(torch.int32).view(n_rows, 18)[:, 16]
        bad = int((st[ok] != 0).sum().item())
        med, step = float(np.median(ms)), float(np.median(step_ms))
        moved = (64 + 72) * n_rows + 4 * clip_ops + 16 * n_desc
        print(json.dumps({
            "what": what, "rows": n_rows, "rows_ok": n_ok, "rows_descriptor": n_desc, "rows_long_form": n_long, "clip_ops": clip_ops,
            "ops_per_ok_row": round(clip_ops / max(n_ok, 1), 1), "self_check_failures": bad, "reps": len(ms), "kernel_ms": round(med, 4),
            "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4), "algorithmic_bytes": moved,
            "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4), "clip_step_ms": round(step, 3), "ratio_to_clip_step": round(med / step, 4)}), flush=True)
        del d_stats, rows, out
        D.last = None

    # ---- config 3: ops by the library's generator, headers from the spans the record scan returns (as bench.py does) ----
    if a.records:
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
        measure(f"config 3, plain: rb_dev_stats_rows behind one liftover step ({n} records, {a.windows} windows)", D, w, POL, None, 14 * n + 1024)
        measure(f"config 3, descriptors: rb_dev_stats_rows behind one liftover step ({n} records, {a.windows} windows)", D, w,
                POL | rustybam_amd.LIFT_DESCRIPTORS, None, 14 * n + 1024)
        del D, d_ops
        torch.cuda.empty_cache()

    # ---- config 4's shape: break-paf --max-size 100 on records of 300-700 ops ----
    if a.records4:
        T, h = config4_resident(torch, eng, dev, a.records4)
        n4 = h["n"]
        D4 = DevBatch.from_device(torch, eng, dev, T.d_ops, h["total_ops"], h["op_off"], [_i64(torch, dev, h[k]) for k in ("t_st", "t_en", "q_st", "q_en")],
                                  torch.from_numpy(h["strand"]).to(dev))
        measure(f"config 4 shape: rb_dev_stats_rows behind break-paf --max-size 100 ({n4} records of 300-700 ops)", D4, None,
                rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | rustybam_amd.BREAK_ONE_WALK, 100, 6 * n4 + 1024)
    eng.close()


if __name__ == "__main__":
    main()
