"""`rb orient [--scaffold]` / `rb filter` on the device text route: the pair call alone, and the commands end to end against another `rb`.

  (a) rb_dev_pairs_records (k_pairs.hip) on --records resident records (the seven columns in HBM, outputs allocated before): warmed, the median
      of --reps calls bracketed by HIP events on the engine's stream.  Two key layouts: MANY (nearly one pair per record: a key per record,
      every tenth record sharing its neighbour's) and FEW (--few-keys keys, record r on key r % few in runs of 4096, every third key on `-`).
      Reported as a fraction of 8 TB/s over its ALGORITHMIC bytes
          45 B per record read (four u64 coordinates, strand, key, q_len) + 4 B per kept record + 16 B per record written (q_st', q_en')
  (b) end to end: `rb orient`, `rb orient --scaffold` and `rb filter --paired-len L` on --e2e-records config-4 records (`rb synth-paf config4`)
      with the query names folded onto --few-keys names and every third query on `-`, from a file and from stdin.  With --against RB (another
      build's `rb`, e.g. the parent commit's) the two binaries run alternately on the same file -- one warm-up, then --rounds rounds, medians --
      and their outputs are compared by md5.  The RB_TIMING phases of one more run each are printed.

One JSON line per case.  No oracle: parity is the business of tests/test_gpu_pairs_records.py and tests/test_gpu_cli_orient_filter.py.

  python tools/bench_pairs_records.py [--records 10000000] [--few-keys 24] [--reps 9] [--e2e-records 200000] [--paired-len 100000] [--against RB]
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
PEAK = 8e12
RB = os.path.join(ROOT, "rustybam_amd", "rb")


def kernel_part(a):
    import torch
    import rustybam_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    n = a.records
    rng = np.random.default_rng(7)
    t_st = rng.integers(0, 1 << 31, n).astype(np.uint64)
    t_en = t_st + rng.integers(1, 20000, n).astype(np.uint64)
    q_st = rng.integers(0, 1 << 20, n).astype(np.uint64)
    q_en = q_st + rng.integers(1, 20000, n).astype(np.uint64)
    q_len = np.full(n, 1 << 22, np.uint64)
    up = lambda x: torch.from_numpy(x.view(np.uint8)).to(dev)  # noqa: E731
    cols = [up(x) for x in (t_st, t_en, q_st, q_en)]
    d_qlen = up(q_len)
    d_kept, d_qs, d_qe = (torch.empty(n * k + 64, dtype=torch.uint8, device=dev) for k in (4, 8, 8))
    d_info = torch.zeros(64, dtype=torch.uint8, device=dev)
    r = np.arange(n)
    layouts = (("many keys (nearly one pair per record)", (r - (r % 10 == 9)).astype(np.uint32), np.where(rng.random(n) < 0.5, ord("+"), ord("-")).astype(np.uint8)),
               (f"few keys ({a.few_keys})", (r // 4096 % a.few_keys).astype(np.uint32), None))
    for what, key, strand in layouts:
        if strand is None:
            strand = np.where(key % 3 == 0, ord("-"), ord("+")).astype(np.uint8)
        n_keys = int(key.max()) + 1
        d_key, d_strand = up(key), up(strand)
        d_flip = torch.zeros(n_keys + 64, dtype=torch.uint8, device=dev)
        d_ord = torch.zeros((n_keys + 8) * 8, dtype=torch.uint8, device=dev)
        d_scr = torch.empty(eng.pairs_records_scratch_bytes(n_keys, n), dtype=torch.uint8, device=dev)
        per_key = np.zeros(n_keys, np.uint64)  # --paired-len: the median of the keys' spans, so half of the keys go and half stay
        np.add.at(per_key, key, t_en - t_st)
        L = int(np.median(per_key))
        torch.cuda.synchronize()
        for mode, mname in ((1, "orient"), (2, "filter"), (3, "orient + filter")):
            ms = []
            for i in range(3 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = eng.dev_pairs_records(*(c.data_ptr() for c in cols), d_strand.data_ptr(), d_key.data_ptr(), d_qlen.data_ptr(), n, n_keys, mode, L, 0, 0,
                                           d_kept.data_ptr(), n, d_qs.data_ptr(), d_qe.data_ptr(), d_flip.data_ptr(), d_ord.data_ptr(), d_info.data_ptr(), d_scr.data_ptr())
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0, rc
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            info = d_info.cpu().numpy().view(rustybam_amd.PAIRS_INFO_DT)[0]
            assert not info["overflow"] and not info["declined"], info
            med, n_kept = float(np.median(ms)), int(info["n_kept"])
            algo = 45 * n + 4 * n_kept + 16 * n
            print(json.dumps({"what": f"rb_dev_pairs_records, {mname}, {what}", "records": n, "keys": n_keys, "kept": n_kept, "flipped_records": int(info["n_flipped_rows"]),
                              "flipped_keys": int(d_flip[:n_keys].sum().item()), "paired_len": L, "reps": a.reps, "call_ms": round(med, 4), "call_ms_min": round(min(ms), 4),
                              "call_ms_max": round(max(ms), 4), "algorithmic_bytes": algo, "fraction_of_8TBps": round(algo / (med * 1e-3) / PEAK, 4)}), flush=True)
    eng.close()


def md5(path):
    hh = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            hh.update(blk)
    return hh.hexdigest()


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
        os.remove(many)

        def run(rb, args, stdin, out, env=None):
            t = time.perf_counter()
            with open(out, "wb") as f:
                if stdin:
                    with open(few, "rb") as src:
                        p = subprocess.run([rb, *args], stdin=src, stdout=f, stderr=subprocess.PIPE, env=env)
                else:
                    p = subprocess.run([rb, *args, few], stdout=f, stderr=subprocess.PIPE, env=env)
            return time.perf_counter() - t, p

        for args in (["orient"], ["orient", "--scaffold"], ["filter", "--paired-len", str(a.paired_len)]):
            for stdin in (False, True):
                o1, o2 = os.path.join(d, "new.txt"), os.path.join(d, "other.txt")
                t1, t2 = [], []
                for i in range(1 + a.rounds):  # the first round warms the page cache and the device
                    s1, p1 = run(RB, args, stdin, o1)
                    assert p1.returncode == 0, p1.stderr[-300:]
                    if a.against:
                        s2, p2 = run(a.against, args, stdin, o2)
                        assert p2.returncode == 0, p2.stderr[-300:]
                    if i:
                        t1.append(s1)
                        if a.against:
                            t2.append(s2)
                res = {"what": f"end to end: rb {' '.join(args)} {'< stdin' if stdin else 'file'} ({a.e2e_records} config-4 records, names folded onto {a.few_keys})",
                       "input_bytes": os.path.getsize(few), "output_bytes": os.path.getsize(o1), "output_lines": sum(1 for _ in open(o1, "rb")), "md5": md5(o1),
                       "seconds": round(float(np.median(t1)), 3), "seconds_all": [round(x, 3) for x in t1]}
                if a.against:
                    res.update({"same_bytes": md5(o1) == md5(o2), "other_seconds": round(float(np.median(t2)), 3), "other_seconds_all": [round(x, 3) for x in t2],
                                "speedup": round(float(np.median(t2)) / float(np.median(t1)), 3)})
                print(json.dumps(res), flush=True)
                for who, rb in (("this build", RB), ("the other build", a.against)):
                    if rb:
                        _, p = run(rb, args, stdin, o2, env={**os.environ, "RB_TIMING": "1"})
                        print(json.dumps({"what": f"RB_TIMING phases, {who}: rb {' '.join(args)} {'< stdin' if stdin else 'file'}",
                                          "stderr": p.stderr.decode(errors="replace").splitlines()}), flush=True)
                assert not a.against or res["same_bytes"], "the two builds printed other bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--few-keys", type=int, default=24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--e2e-records", type=int, default=200_000)
    ap.add_argument("--paired-len", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--against", default=None, help="another build's rb to run alternately (its library beside it)")
    a = ap.parse_args()
    if a.records:
        kernel_part(a)
    if a.e2e_records:
        e2e_part(a)


if __name__ == "__main__":
    main()
