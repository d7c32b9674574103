"""`rb break-paf --orient --paired-len L`: the pair call alone, and the one-command pipeline against the piped commands it replaces.

  (a) rb_dev_pairs_rows (k_pairs.hip) on the hit rows of one break-paf step where they lie in HBM: --records config-4-shaped records (300-700
      synthetic ops, four records per query, random strands) broken with --max-size, in descriptor mode (what the pipeline uses).  The call
      (rows_cap = every row, outputs allocated before) is bracketed by HIP events on the engine's stream: warmed, the median of --reps calls.
      Twice: with FEW keys (--few-keys of them, in runs of n / few records: every adder of a wavefront on one address) and with MANY (one key
      per four records, config 4's shape).  Reported as a fraction of 8 TB/s over its ALGORITHMIC bytes
          64 B per row read + 64 B per kept row written + 13 B per record (key 4, q_len 8, strand 1)
      with, beside it, the bytes its three passes move as written (each pass reads the rows again: 3 x 64 B per row, 24 B per row of keep
      counts written, scanned and read, 64 B per kept row).  Yardstick of the same run on the same rows and batch: rb_dev_stats_rows
      ((64 + 72) B per row, 4 B per op, 16 B per descriptor).
  (b) end to end: `rb break-paf --max-size N --orient --paired-len L --stats` on --e2e-records config-4 records (`rb synth-paf config4`)
      against `rb break-paf --max-size N | rb orient - | rb filter --paired-len L - | rb stats --paf -` (code the options do not touch) on
      the same file: same bytes out, wall time of each, warmed, the median of three.  Twice: the file as generated (nearly one (target,
      query) pair per record, every record on `+`) and with its query names folded onto --few-keys names and every third query on `-`.

One JSON line per case.  No oracle: parity is the business of tests/test_gpu_pairs_rows.py and tests/test_gpu_cli_pairs.py.

  python tools/bench_pairs.py [--records 2000000] [--max-size 10] [--few-keys 24] [--reps 9] [--e2e-records 200000] [--paired-len 100000]
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
    from devutil import DevBatch, _i64, config4_resident
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

    T, h = config4_resident(torch, eng, dev, a.records)
    n = h["n"]
    D = DevBatch.from_device(torch, eng, dev, T.d_ops, h["total_ops"], h["op_off"], T.d_c, T.d_strand)
    policy = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | rustybam_amd.LIFT_DESCRIPTORS
    rows, out, cnt = D.run(None, policy=policy, max_size=a.max_size, rows_cap=8 * n + 1024)
    n_rows = int(cnt["n_hits"])
    n_ops = int(rows[:, 3].to(torch.int64).sum().item())
    n_desc = int(((rows[:, 2] & 0xFFFF) == 0).logical_and(((rows[:, 2] >> 16) & rustybam_amd.HIT_DESCRIPTOR) != 0).sum().item())
    q_len = np.full(n, int(h["q_en"].max()) + 1000, np.uint64)
    d_qlen = _i64(torch, dev, q_len)
    d_out = torch.empty((n_rows + 1) * 64, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_stats = torch.empty((n_rows + 1) * 72, dtype=torch.uint8, device=dev)
    s_med, _, _ = timed(lambda: eng.dev_stats_rows(D.view, rows.data_ptr(), n_rows, out.data_ptr(), d_stats.data_ptr()))
    s_moved = (64 + 72) * n_rows + 4 * n_ops + 16 * n_desc
    h_rows = rows.cpu().numpy().view(np.uint8).reshape(-1).view(rustybam_amd.HIT_DT)
    h_rows = h_rows[h_rows["status"] == 0]  # (a few rows are the reference's None: they count nowhere)
    for what, key in ((f"few keys ({a.few_keys})", (np.arange(n) * a.few_keys // n).astype(np.uint32)), ("many keys (one per 4 records)", (np.arange(n) // 4).astype(np.uint32))):
        n_keys = int(key.max()) + 1
        d_key = torch.from_numpy(key.view(np.int32)).to(dev)
        d_flip = torch.zeros(n_keys + 64, dtype=torch.uint8, device=dev)
        d_scr = torch.empty(eng.pairs_scratch_bytes(n_keys, n_rows), dtype=torch.uint8, device=dev)
        per_key = np.zeros(n_keys, np.uint64)  # --paired-len: the median of the keys' piece spans, so half of the keys go and half stay
        np.add.at(per_key, key[h_rows["rec"]], h_rows["t_en"] - h_rows["t_st"])
        L = int(np.median(per_key))
        torch.cuda.synchronize()
        for mode, mname in ((3, "orient + filter"), (1, "orient"), (2, "filter")):
            med, lo, hi = timed(lambda: eng.dev_pairs_rows(rows.data_ptr(), n_rows, d_key.data_ptr(), d_qlen.data_ptr(), T.d_strand.data_ptr(), n, n_keys, mode,
                                                           L, 0, 0, d_out.data_ptr(), n_rows, d_flip.data_ptr(), d_info.data_ptr(), d_scr.data_ptr()))
            info = d_info.cpu().numpy().view(rustybam_amd.PAIRS_INFO_DT)[0]
            assert not info["overflow"] and not info["declined"], info
            n_kept = int(info["n_kept"])
            algo = 64 * n_rows + 64 * n_kept + 13 * n
            moved = 3 * 64 * n_rows + 24 * n_rows + 64 * n_kept + 13 * n
            print(json.dumps({
                "what": f"rb_dev_pairs_rows, {mname}, {what}, behind break-paf --max-size {a.max_size} ({n} config-4 records)",
                "rows": n_rows, "keys": n_keys, "kept": n_kept, "flipped_rows": int(info["n_flipped_rows"]), "flipped_keys": int(d_flip[:n_keys].sum().item()),
                "paired_len": L, "reps": a.reps, "call_ms": round(med, 4), "call_ms_min": round(lo, 4), "call_ms_max": round(hi, 4),
                "algorithmic_bytes": algo, "fraction_of_8TBps": round(algo / (med * 1e-3) / PEAK, 4),
                "bytes_as_written": moved, "fraction_of_8TBps_as_written": round(moved / (med * 1e-3) / PEAK, 4),
                "yardstick_stats_rows_ms": round(s_med, 4), "yardstick_stats_rows_fraction": round(s_moved / (s_med * 1e-3) / PEAK, 4)}), flush=True)
    eng.close()


def e2e_part(a):
    with tempfile.TemporaryDirectory() as d:
        many, few = os.path.join(d, "many.paf"), os.path.join(d, "few.paf")
        with open(many, "wb") as f:
            subprocess.check_call([RB, "synth-paf", "config4", str(a.e2e_records)], stdout=f)
        with open(many, "rb") as f, open(few, "wb") as g:  # the same records: query q<k> becomes q<k % few>, every third of those on `-`
            for ln in f:
                t = ln.split(b"\t", 5)
                k = int(t[0][1:]) % a.few_keys
                t[0], t[4] = b"q%d" % k, b"-" if k % 3 == 0 else b"+"
                g.write(b"\t".join(t))
        n, L = str(a.max_size), str(a.paired_len)

        def one(paf, out):
            t = time.perf_counter()
            with open(out, "wb") as f:
                rc = subprocess.call([RB, "break-paf", "--max-size", n, "--orient", "--paired-len", L, "--stats", paf], stdout=f)
            return time.perf_counter() - t, rc

        def piped(paf, out):
            t = time.perf_counter()
            with open(out, "wb") as f:
                p1 = subprocess.Popen([RB, "break-paf", "--max-size", n, paf], stdout=subprocess.PIPE)
                p2 = subprocess.Popen([RB, "orient", "-"], stdin=p1.stdout, stdout=subprocess.PIPE)
                p3 = subprocess.Popen([RB, "filter", "--paired-len", L, "-"], stdin=p2.stdout, stdout=subprocess.PIPE)
                p4 = subprocess.Popen([RB, "stats", "--paf", "-"], stdin=p3.stdout, stdout=f)
                p1.stdout.close(), p2.stdout.close(), p3.stdout.close()
                rcs = [p4.wait(), p3.wait(), p2.wait(), p1.wait()]
            return time.perf_counter() - t, max(rcs)

        def md5(path):
            hh = hashlib.md5()
            with open(path, "rb") as f:
                for blk in iter(lambda: f.read(1 << 24), b""):
                    hh.update(blk)
            return hh.hexdigest()
        for what, paf in (("many pairs (the file as generated)", many), (f"few pairs ({a.few_keys} query names)", few)):
            o1, o2 = os.path.join(d, "one.txt"), os.path.join(d, "piped.txt")
            t1, t2 = [], []
            for i in range(4):  # the first round warms the page cache and the device
                (s1, rc1), (s2, rc2) = one(paf, o1), piped(paf, o2)
                assert rc1 == 0 and rc2 == 0, (rc1, rc2)
                if i:
                    t1.append(s1), t2.append(s2)
            same = md5(o1) == md5(o2)
            print(json.dumps({"what": f"end to end, {what}: rb break-paf --max-size {n} --orient --paired-len {L} --stats against rb break-paf | rb orient - | "
                                      f"rb filter --paired-len {L} - | rb stats --paf - ({a.e2e_records} config-4 records)",
                              "input_bytes": os.path.getsize(paf), "output_bytes": os.path.getsize(o1), "output_lines": sum(1 for _ in open(o1, "rb")),
                              "same_bytes": same, "one_command_s": round(float(np.median(t1)), 3), "one_command_all": [round(x, 3) for x in t1],
                              "four_commands_s": round(float(np.median(t2)), 3), "four_commands_all": [round(x, 3) for x in t2],
                              "speedup": round(float(np.median(t2)) / float(np.median(t1)), 3)}), flush=True)
            assert same, "the one-command form printed other bytes than the pipeline"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--max-size", type=int, default=10)
    ap.add_argument("--few-keys", type=int, default=24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--e2e-records", type=int, default=200_000)
    ap.add_argument("--paired-len", type=int, default=100_000)
    a = ap.parse_args()
    if a.records:
        kernel_part(a)
    if a.e2e_records:
        e2e_part(a)


if __name__ == "__main__":
    main()
