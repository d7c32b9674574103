"""`rb nucfreq` with the lines printed on the device: (a) rb_dev_nucfreq_text (k_nftext.hip) alone, (b) `rb nucfreq` end to end.

  (a) kernel   counts of --positions positions at 30x resident in HBM (a majority base of 28 to 30, the rest spread; every position
               covered), cut into print pieces of 1 Mbp as the front end cuts them, prefix `chrS` TAB and suffix TAB `chrS:1-N` LF.  Both
               modes; the sizes-only call and the full call are each bracketed by HIP events on the engine's stream with the outputs
               allocated before: warmed, the median of --reps calls with min and max.  Beside it the time the text takes from the
               device into page-locked host memory (one copy, HIP events), the transfer the call feeds.  One JSON line per mode with
               the bytes moved: 16 B per position read twice (sizes, print) and the text written, as a fraction of 8 TB/s.
  (b) end to end  tools/gen_config5_bam.py --e2e N written once, then `rb nucfreq -r chrS:1-N [-s]` into a file by the text route, by the
               host formatter (RB_GENERAL_PATH=1) and -- with --against RB, another build's `rb` with its library beside it, e.g. the
               parent commit's -- by that build, alternately: one first run each, then --rounds rounds, medians with min and max, the
               outputs compared by digest.  The pass mark of a format: the text route's median below the other build's median by more
               than the other build's own min-to-max spread.  The RB_TIMING laps of one more run of the text route are printed.

No oracle here: parity is the business of tests/test_gpu_nucfreq_text.py and tests/test_gpu_cli_nucfreq_text.py.

  python tools/bench_nucfreq_text.py [--positions 20000000] [--reps 20] [--e2e 20000000] [--rounds 5] [--against RB] [--tmp DIR]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PEAK = 8e12
PIECE = 1000000


def kernel(a):
    import torch
    import rustybam_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    n = a.positions
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    major = torch.randint(0, 4, (n,), device=dev, generator=g)
    top = torch.randint(28, 31, (n,), device=dev, generator=g, dtype=torch.int32)
    counts = torch.zeros((n + 4, 4), dtype=torch.int32, device=dev)
    counts[:n].scatter_(1, major[:, None], top[:, None])
    counts[:n].scatter_add_(1, ((major + 1 + torch.randint(0, 3, (n,), device=dev, generator=g)) % 4)[:, None], (30 - top)[:, None])
    counts[:n, 0] |= -0x80000000  # RB_NF_COVERED
    del major, top
    seg_pos = np.arange(0, n, PIECE, dtype=np.uint64)
    seg_n = np.minimum(n - seg_pos, PIECE).astype(np.uint32)
    n_seg = len(seg_n)
    strings = b"chrS\t" + b"\tchrS:1-%d\n" % n
    d_str = torch.from_numpy(np.frombuffer(strings, np.uint8).copy()).to(dev)
    u32 = lambda v: np.full(n_seg, v, np.uint32)  # noqa: E731
    pre_off, pre_len, suf_off, suf_len = u32(0), u32(5), u32(5), u32(len(strings) - 5)
    d_off = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    d_first = torch.zeros(n_seg, dtype=torch.int64, device=dev)
    d_lines = torch.zeros(n_seg, dtype=torch.int64, device=dev)
    scr = torch.zeros(eng.nucfreq_text_scratch_bytes(n_seg, n) + 512, dtype=torch.uint8, device=dev)
    d_scr = (scr.data_ptr() + 255) & ~255

    def timed(fn):
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)

    for mode, what in ((rustybam_amd.NFT_FULL, "full lines"), (rustybam_amd.NFT_SMALL, "--small lines")):
        def call(text, cap):
            eng.dev_nucfreq_text(counts.data_ptr(), seg_pos, seg_pos, seg_n, d_str.data_ptr(), pre_off, pre_len, suf_off, suf_len, mode, d_off.data_ptr(),
                                 d_first.data_ptr(), d_lines.data_ptr(), text, cap, d_scr)
        torch.cuda.synchronize()
        call(0, 0)
        torch.cuda.synchronize()
        total = int(d_off[n_seg].item())
        assert int(d_lines.sum().item()) == n
        text = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        host = torch.empty(total, dtype=torch.uint8).pin_memory()
        sizes = timed(lambda: call(0, 0))
        full = timed(lambda: call(text.data_ptr(), total))
        copy = timed(lambda: host.copy_(text[:total], non_blocking=True))
        head = bytes(host[:120].numpy()).split(b"\n")[:2]
        moved = 2 * 16 * n + total
        print(json.dumps({"what": f"rb_dev_nucfreq_text, {what}", "shape": rustybam_amd.nucfreq_text_shape(), "positions": n, "segments": n_seg, "reps": a.reps,
                          "text_bytes": total, "bytes_per_position": round(total / n, 2), "counts_bytes_read": 2 * 16 * n,
                          "call_ms": full[0], "call_ms_min": full[1], "call_ms_max": full[2], "sizes_only_ms": sizes[0],
                          "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (full[0] * 1e-3) / PEAK, 4),
                          "text_download_ms": copy[0], "text_download_ms_min": copy[1], "text_download_ms_max": copy[2],
                          "counts_download_bytes_of_the_host_route": 16 * n, "first_lines": [x.decode() for x in head]}), flush=True)
        del text, host
        torch.cuda.empty_cache()
    eng.close()


def md5_file(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def end_to_end(a):
    import tempfile
    rb = os.path.join(ROOT, "rustybam_amd", "rb")
    n = a.e2e
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        bam = os.path.join(d, "c5.bam")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_config5_bam.py"), str(n), bam])
        for fmt, extra in (("full lines", []), ("--small", ["-s"])):
            routes = [("text route", rb, {}), ("host formatter (RB_GENERAL_PATH=1)", rb, {"RB_GENERAL_PATH": "1"})]
            if a.against:
                routes.append(("the other build", a.against, {}))
            secs, digest, size = {r[0]: [] for r in routes}, {}, 0
            for i in range(1 + a.rounds):  # the first round warms the page cache and the device
                for who, exe, env in routes:
                    out = os.path.join(d, "out.txt")
                    with open(out, "wb") as f:
                        t0 = time.perf_counter()
                        r = subprocess.run([exe, "nucfreq", "-r", f"chrS:1-{n}", *extra, bam], stdout=f, stderr=subprocess.DEVNULL, env={**os.environ, **env})
                        dt = time.perf_counter() - t0
                    assert r.returncode == 0, who
                    if i == 0:
                        digest[who], size = md5_file(out), os.path.getsize(out)
                    else:
                        secs[who].append(dt)
                    os.unlink(out)
            res = {"what": f"end to end: rb nucfreq -r chrS:1-{n} ({fmt})", "positions": n, "input_bytes": os.path.getsize(bam), "output_bytes": size,
                   "md5": digest["text route"], "rounds": a.rounds, "cpus": len(os.sched_getaffinity(0))}
            for who in secs:
                s = secs[who]
                res[who] = {"seconds_median": round(float(np.median(s)), 4), "seconds_min": round(min(s), 4), "seconds_max": round(max(s), 4),
                            "same_bytes": digest[who] == digest["text route"]}
            if a.against:
                o = res["the other build"]
                spread = o["seconds_max"] - o["seconds_min"]
                res["pass_mark"] = {"other_median_minus_text_route_median": round(o["seconds_median"] - res["text route"]["seconds_median"], 4),
                                    "other_min_to_max_spread": round(spread, 4),
                                    "met": res["text route"]["seconds_median"] < o["seconds_median"] - spread}
            print(json.dumps(res), flush=True)
            p = subprocess.run([rb, "nucfreq", "-r", f"chrS:1-{n}", *extra, bam], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env={**os.environ, "RB_TIMING": "1"})
            print(json.dumps({"what": f"RB_TIMING laps, text route ({fmt}, {n} positions, output to /dev/null)", "stderr": p.stderr.decode(errors="replace").splitlines()}), flush=True)
            assert len(set(digest.values())) == 1, "the routes printed other bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--against", default=None, help="another build's rb to run alternately (its library beside it)")
    ap.add_argument("--tmp", default=None, help="where the BAM and the outputs are written (default: the system's temporary directory)")
    a = ap.parse_args()
    if a.positions:
        kernel(a)
    if a.e2e:
        end_to_end(a)


if __name__ == "__main__":
    main()
