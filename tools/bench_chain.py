"""`rb liftover --break`: the link kernel alone, and the one-command pipeline against the two commands it replaces.

  (a) rb_dev_rows_to_batch (k_rows_batch.hip) on the hit rows of one break-paf step where they lie in HBM: bench.py's config-3 records
      (--records synthetic records of 1000-9000 ops, seed 0x5EED0003) broken with every --max-size given, in descriptor mode (what the
      pipeline uses) and plain.  The fill call (sizes known) is bracketed by HIP events on the engine's stream with its outputs allocated
      before: warmed, the median of --reps calls.  Reported as a fraction of 8 TB/s over its algorithmic bytes: 64 B per row, 8 B per op
      (4 read, 4 written), 54 B of header per piece (49 written, 5 read), 16 B per descriptor.  Yardsticks of the same run, on the same rows and batch:
      rb_dev_stats_rows (64 + 72 B per row, 4 B per op, 16 B per descriptor) and the in-place rb_dev_swap (8 B per op).
  (b) end to end: `rb liftover --bed W --break N` on --e2e-records synthetic records x --windows windows against
      `rb break-paf --max-size N | rb liftover --bed W -` (code the option does not touch) on the same file: same bytes out, wall time of
      each, warmed, the median of three.

One JSON line per case.  No oracle: parity is the business of tests/test_gpu_rows_to_batch.py and tests/test_gpu_cli_chain.py.

  python tools/bench_chain.py [--records 200000] [--max-size 1000 10] [--reps 9] [--e2e-records 100000] [--windows 3000]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK = 8e12
RB = os.path.join(ROOT, "rustybam_amd", "rb")


def kernel_part(a):
    import torch
    import rustybam_amd
    from rustybam_amd import workload as wl
    from devutil import DevBatch, _i64
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(fn):
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = ev(), ev()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms)

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
    D = DevBatch.from_device(torch, eng, dev, d_ops, total_ops, off, [_i64(torch, dev, x) for x in (t_st, t_en, q_st, q_en)], torch.from_numpy(strand).to(dev))
    for max_size in a.max_size:
        for desc in (True, False):
            policy = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | (rustybam_amd.LIFT_DESCRIPTORS if desc else rustybam_amd.BREAK_ONE_WALK)
            rows, out, cnt = D.run(None, policy=policy, max_size=max_size, rows_cap=8 * n + 1024)
            n_rows = int(cnt["n_hits"])
            d_scr = torch.empty(eng.rows_to_batch_scratch_bytes(n_rows), dtype=torch.uint8, device=dev)
            d_info = torch.zeros(64, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            eng.dev_rows_to_batch(D.view, rows.data_ptr(), n_rows, out.data_ptr(), 0, 0, 0, 0, None, 0, 0, 0, d_info.data_ptr(), d_scr.data_ptr())
            torch.cuda.synchronize()
            info = d_info.cpu().numpy().view(rustybam_amd.PIECES_INFO_DT)[0]
            n_p, n_o = int(info["n_pieces"]), int(info["n_ops"])
            d_new = torch.empty(n_o + 64, dtype=torch.int32, device=dev)
            d_poff = torch.empty(n_p + 1, dtype=torch.int64, device=dev)
            d_c = [torch.empty(n_p, dtype=torch.int64, device=dev) for _ in range(4)]
            d_s, d_ct, d_par = torch.empty(n_p, dtype=torch.uint8, device=dev), torch.empty(n_p, dtype=torch.int32, device=dev), torch.empty(n_p, dtype=torch.int32, device=dev)
            d_stats = torch.empty((n_rows + 1) * 72, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            med, lo, hi = timed(lambda: eng.dev_rows_to_batch(D.view, rows.data_ptr(), n_rows, out.data_ptr(), n_p, n_o, d_new.data_ptr(), d_poff.data_ptr(),
                                                              [x.data_ptr() for x in d_c], d_s.data_ptr(), d_ct.data_ptr(), d_par.data_ptr(), d_info.data_ptr(),
                                                              d_scr.data_ptr()))
            info = d_info.cpu().numpy().view(rustybam_amd.PIECES_INFO_DT)[0]
            assert not info["overflow"] and int(d_poff[n_p].item()) == n_o
            ok = (rows[:, 2] & 0xFFFF) == 0
            is_desc = ((rows[:, 2] >> 16) & rustybam_amd.HIT_DESCRIPTOR) != 0
            n_desc = int((ok & is_desc).sum().item())
            per = torch.diff(d_poff)
            n_long = int((per > rustybam_amd.capi.rows_to_batch_shape()[1]).sum().item())
            moved = 64 * n_rows + 8 * n_o + 54 * n_p + 16 * n_desc
            s_med, _, _ = timed(lambda: eng.dev_stats_rows(D.view, rows.data_ptr(), n_rows, out.data_ptr(), d_stats.data_ptr()))
            s_moved = (64 + 72) * n_rows + 4 * n_o + 16 * n_desc
            print(json.dumps({
                "what": f"rb_dev_rows_to_batch behind break-paf --max-size {max_size}, {'descriptors' if desc else 'plain ops'} ({n} config-3 records)",
                "rows": n_rows, "pieces": n_p, "piece_ops": n_o, "ops_per_piece": round(n_o / max(n_p, 1), 1), "pieces_long_form": n_long, "rows_descriptor": n_desc,
                "declined": int(info["declined"]), "reps": a.reps, "kernel_ms": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4),
                "yardstick_stats_rows_ms": round(s_med, 4), "yardstick_stats_rows_fraction": round(s_moved / (s_med * 1e-3) / PEAK, 4)}), flush=True)
            del d_new, d_poff, d_c, d_s, d_ct, d_par, d_stats, d_scr, rows, out
            D.last = None
            torch.cuda.empty_cache()
    # the other yardstick: the in-place swap of the same batch (twice restores it)
    w_med, _, _ = timed(lambda: eng.dev_swap(D.view, d_ops.data_ptr()))
    print(json.dumps({"what": f"yardstick: rb_dev_swap in place ({n} config-3 records)", "ops": total_ops, "kernel_ms": round(w_med, 4),
                      "fraction_of_8TBps": round(8 * total_ops / (w_med * 1e-3) / PEAK, 4)}), flush=True)
    eng.close()


def e2e_part(a):
    with tempfile.TemporaryDirectory() as d:
        paf, bed = os.path.join(d, "in.paf"), os.path.join(d, "w.bed")
        with open(paf, "wb") as f:
            subprocess.check_call([RB, "synth-paf", str(0x5EED0003), "0", str(a.e2e_records)], stdout=f)
        with open(bed, "wb") as f:
            subprocess.check_call([RB, "synth-bed", str(a.windows)], stdout=f)
        n = str(a.e2e_max_size)

        def one(out):
            t = time.perf_counter()
            with open(out, "wb") as f:
                rc = subprocess.call([RB, "liftover", "--bed", bed, "--break", n, paf], stdout=f)
            return time.perf_counter() - t, rc

        def two(out):
            t = time.perf_counter()
            with open(out, "wb") as f:
                p1 = subprocess.Popen([RB, "break-paf", "--max-size", n, paf], stdout=subprocess.PIPE)
                p2 = subprocess.Popen([RB, "liftover", "--bed", bed, "-"], stdin=p1.stdout, stdout=f)
                p1.stdout.close()
                rc2, rc1 = p2.wait(), p1.wait()
            return time.perf_counter() - t, rc1 or rc2

        def md5(path):
            h = hashlib.md5()
            with open(path, "rb") as f:
                for blk in iter(lambda: f.read(1 << 24), b""):
                    h.update(blk)
            return h.hexdigest()
        o1, o2 = os.path.join(d, "one.paf"), os.path.join(d, "two.paf")
        t1, t2 = [], []
        for i in range(4):  # the first round warms the page cache and the device
            (s1, rc1), (s2, rc2) = one(o1), two(o2)
            assert rc1 == 0 and rc2 == 0, (rc1, rc2)
            if i:
                t1.append(s1), t2.append(s2)
        same = md5(o1) == md5(o2)
        print(json.dumps({"what": f"end to end: rb liftover --bed W --break {n} against rb break-paf --max-size {n} | rb liftover --bed W - "
                                  f"({a.e2e_records} synthetic records, {a.windows} windows)",
                          "input_bytes": os.path.getsize(paf), "output_bytes": os.path.getsize(o1), "same_bytes": same,
                          "one_command_s": round(float(np.median(t1)), 3), "one_command_all": [round(x, 3) for x in t1],
                          "two_commands_s": round(float(np.median(t2)), 3), "two_commands_all": [round(x, 3) for x in t2],
                          "speedup": round(float(np.median(t2)) / float(np.median(t1)), 3)}), flush=True)
        assert same, "the one-command form printed other bytes than the pipeline"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--max-size", type=int, nargs="+", default=[1000, 10])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--e2e-records", type=int, default=100_000)
    ap.add_argument("--e2e-max-size", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=3000)
    a = ap.parse_args()
    if a.records:
        kernel_part(a)
    if a.e2e_records:
        e2e_part(a)


if __name__ == "__main__":
    main()
