"""`rb nucfreq` with the BAM decoded on the device: (a) rb_dev_bam_reads (k_bamreads.hip) alone, (b) `rb nucfreq` end to end.

  (a) kernel   the columns of rb_dev_bam_records resident in HBM, synthetic: --records records of 1 to 5 ops, and --long-records records of
               about 3000 ops.  The call is bracketed by HIP events on the engine's stream with outputs and scratch allocated before:
               warmed, the median of --reps calls with min and max.  One JSON line per shape with the algorithmic bytes (per record 37 B
               of columns and record place + 8 B of fixed fields + 4 B per op in, 24 B out, and the scan's 24 B) as a fraction of 8 TB/s.
  (b) end to end  two files of --e2e bp at 30x, written once with their .bai: 15 kb reads (the shape of tools/gen_config5_bam.py) and
               150-base reads.  `rb nucfreq -r chrS:1-N` in both formats, with the index and with RB_NO_BAI=1, by three commands
               alternately -- this build on the device route (RB_NUCFREQ_DEV_DECODE=1), this build with RB_GENERAL_PATH=1, and with
               --against RB another build's `rb` with its library beside it, e.g. the parent commit's --: one first run each, then
               --rounds rounds, medians with min and max, the outputs compared by digest.  The pass mark of a line (format x file x
               index): the device route's median does not exceed the other build's median by more than the other build's own min-to-max
               spread.  The RB_TIMING laps of one more run of the device route per file are printed.

No oracle here: parity is the business of tests/test_gpu_bam_reads.py and tests/test_gpu_cli_nucfreq_bam.py.

  python tools/bench_nucfreq_bam.py [--records 10000000] [--long-records 100000] [--reps 20] [--e2e 20000000] [--rounds 5] [--against RB] [--tmp DIR]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_nucfreq import make_reads, SEED  # noqa: E402
from bench_nucfreq_text import md5_file     # noqa: E402
PEAK = 8e12
STRIDE = 48  # bytes from one synthetic record to the next: its block_size field, the fixed fields, a short name


def kernel(a):
    import torch
    import rustybam_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for what, n, lo, hi in (("1-5 ops", a.records, 1, 6), ("~3000 ops", a.long_records, 2900, 3100)):
        if not n:
            continue
        n_ops = torch.randint(lo, hi, (n,), device=dev, generator=g, dtype=torch.int64)
        op_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        op_off[1:] = torch.cumsum(n_ops, 0)
        total = int(op_off[n])
        ops = (torch.randint(1, 200, (total + 4,), device=dev, generator=g, dtype=torch.int32) << 4) | torch.tensor([0, 0, 0, 1, 2, 7, 8, 4], dtype=torch.int32, device=dev)[
            torch.randint(0, 8, (total + 4,), device=dev, generator=g)]
        data = torch.zeros(n * STRIDE + 32, dtype=torch.uint8, device=dev)
        data[12::STRIDE][:n] = 2  # l_read_name; (n_cigar_op only moves seq_off: the ops come from the ops array)
        rec_off = torch.arange(n, dtype=torch.int64, device=dev) * STRIDE + 4
        rec_len = torch.full((n,), STRIDE - 4, dtype=torch.int32, device=dev)
        tid = torch.zeros(n, dtype=torch.int32, device=dev)
        pos = torch.cumsum(torch.randint(0, 8, (n,), device=dev, generator=g, dtype=torch.int64), 0)
        flag = torch.where(torch.rand(n, device=dev, generator=g) < 0.02, 0x400, 0).to(torch.int32)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        out = [torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(3)]
        fu = torch.zeros(1, dtype=torch.int64, device=dev)
        scr = torch.zeros(eng.bam_reads_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev)
        sp = (scr.data_ptr() + 255) & ~255
        args = (data.data_ptr(), rec_off.data_ptr(), rec_len.data_ptr(), n, tid.data_ptr(), pos.data_ptr(), flag.data_ptr(), op_off.data_ptr(), ops.data_ptr(),
                status.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), fu.data_ptr(), sp)
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.dev_bam_reads(*args)
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        assert int(fu[0]) == -1 and bool((out[2][1:n] >= out[2][:n - 1]).all())
        moved = n * (37 + 8 + 24 + 24) + 4 * total
        med = float(np.median(ms))
        print(json.dumps({"what": f"rb_dev_bam_reads alone, {what}", "records": n, "ops": total, "reps": a.reps, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4), "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}), flush=True)
        del n_ops, op_off, ops, data, rec_off, rec_len, tid, pos, flag, status, out, scr
        torch.cuda.empty_cache()
    eng.close()


# ---- a coordinate-sorted BGZF BAM of one contig chrS with its .bai: records of one size, built column-wise ----
def gen_bam(contig, read_len, path):
    pos, ops, op_off, n = make_reads(contig, 30, read_len)
    nop = int(op_off[1] - op_off[0])
    ops = ops.reshape(n, nop)
    rng = np.random.default_rng(SEED)
    codes = np.array([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88], np.uint8)
    sb = (read_len + 1) // 2
    dt = np.dtype([("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("l_rn", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"), ("l_seq", "<u4"),
                   ("next", "<i4", (3,)), ("name", "S10"), ("ops", "<u4", (nop,)), ("seq", "u1", (sb,)), ("qual", "u1", (read_len,))])
    head = b"BAM\x01"
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrS\tLN:%d\n" % contig
    head += struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrS\0" + struct.pack("<i", contig)
    ref_len = ((ops >> 4) * np.isin(ops & 15, [0, 2])).sum(axis=1).astype(np.int64)
    coff, at = [], 0          # file offset of every BGZF member; members of 0xFF00 bytes of the stream
    carry = head
    with open(path, "wb") as f:
        def put(buf, last):
            nonlocal at
            k = len(buf) if last else len(buf) // 0xFF00 * 0xFF00
            for o in range(0, k, 0xFF00):
                chunk = buf[o:o + 0xFF00]
                co = zlib.compressobj(1, zlib.DEFLATED, -15)
                comp = co.compress(chunk) + co.flush()
                coff.append(at)
                blk = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk))
                f.write(blk)
                at += len(blk)
            return buf[k:]
        step = max((64 << 20) // dt.itemsize, 1)  # (64 MiB of records at a time: the raw stream of the long reads is 0.9 GB)
        for r0 in range(0, n, step):
            r1 = min(r0 + step, n)
            rec = np.zeros(r1 - r0, dt)
            rec["bs"], rec["pos"], rec["l_rn"], rec["mapq"], rec["n_cig"], rec["l_seq"] = dt.itemsize - 4, pos[r0:r1], 10, 60, nop, read_len
            rec["next"] = (-1, -1, 0)
            rec["name"] = np.char.add("r", np.char.zfill(np.arange(r0, r1).astype(str), 8)).astype("S9")
            rec["ops"], rec["qual"] = ops[r0:r1], 0xFF
            rec["seq"] = codes[rng.integers(0, 16, (r1 - r0, sb))]
            carry = put(carry + rec.tobytes(), False)
        put(carry, True)
        coff.append(at)
        f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0")  # the empty end-of-file member
    # the .bai (SAM spec 5.2): bins of chunks of virtual offsets + the 16 kb linear index
    start = len(head) + dt.itemsize * np.arange(n + 1, dtype=np.int64)
    voff = (np.array(coff, np.int64)[start // 0xFF00] << 16) | (start % 0xFF00)
    b, e = pos, pos + ref_len
    bins = np.zeros(n, np.int64)
    done = np.zeros(n, bool)
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & ((b >> shift) == ((e - 1) >> shift))
        bins[hit] = base + (b[hit] >> shift)
        done |= hit
    run0 = np.concatenate([[0], np.flatnonzero(bins[1:] != bins[:-1]) + 1])
    run1 = np.concatenate([run0[1:], [n]])
    chunks = {}
    for r0, r1 in zip(run0.tolist(), run1.tolist()):
        chunks.setdefault(int(bins[r0]), []).append((int(voff[r0]), int(voff[r1])))
    n_intv = int((e.max() - 1) >> 14) + 1
    w0 = np.arange(n_intv, dtype=np.int64) << 14
    first = np.searchsorted(np.maximum.accumulate(e), w0, side="right")  # the first record that ends behind the window's start
    io = np.where((first < n) & (b[np.minimum(first, n - 1)] < w0 + (1 << 14)), voff[np.minimum(first, n - 1)], 0)
    for w in range(n_intv - 2, -1, -1):  # windows nobody overlaps take the next window's offset, as samtools writes them
        if io[w] == 0:
            io[w] = io[w + 1]
    with open(path + ".bai", "wb") as f:
        f.write(b"BAI\x01" + struct.pack("<i", 1) + struct.pack("<i", len(chunks)))
        for k, ch in chunks.items():
            f.write(struct.pack("<Ii", k, len(ch)) + b"".join(struct.pack("<QQ", x, y) for x, y in ch))
        f.write(struct.pack("<i", n_intv) + io.astype("<u8").tobytes())
    return n


def end_to_end(a):
    import tempfile
    rb = os.path.join(ROOT, "rustybam_amd", "rb")
    n = a.e2e
    passed = []
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        for read_len in (15000, 150):
            bam = os.path.join(d, f"reads{read_len}.bam")
            t0 = time.perf_counter()
            n_reads = gen_bam(n, read_len, bam)
            print(json.dumps({"what": f"file of {read_len}-base reads", "reads": n_reads, "bytes": os.path.getsize(bam), "seconds_to_write": round(time.perf_counter() - t0, 1)}), flush=True)
            for index, ienv in (("indexed", {}), ("RB_NO_BAI=1", {"RB_NO_BAI": "1"})):
                for fmt, extra in (("full lines", []), ("--small", ["-s"])):
                    fenv = {**ienv, **({} if extra else {"RB_NUCFREQ_TEXT": "1"})}
                    routes = [("device route", rb, {**fenv, "RB_NUCFREQ_DEV_DECODE": "1"}), ("host decode (RB_GENERAL_PATH=1)", rb, {**ienv, "RB_GENERAL_PATH": "1"})]
                    if a.against:
                        routes.append(("the other build", a.against, fenv))
                    secs, digest, size = {r[0]: [] for r in routes}, {}, 0
                    for i in range(1 + a.rounds):  # the first round warms the page cache and the device
                        for who, exe, env in routes:
                            out = os.path.join(d, "out.txt")
                            with open(out, "wb") as f:
                                t0 = time.perf_counter()
                                r = subprocess.run([exe, "nucfreq", "-r", f"chrS:1-{n}", *extra, bam], stdout=f, stderr=subprocess.PIPE, env={**os.environ, **env})
                                dt = time.perf_counter() - t0
                            if r.returncode != 0:  # (nothing more is started after a run that failed)
                                raise SystemExit(f"{who} ended with {r.returncode}: {r.stderr[-400:]!r}")
                            if i == 0:
                                digest[who], size = md5_file(out), os.path.getsize(out)
                            else:
                                secs[who].append(dt)
                            os.unlink(out)
                    res = {"what": f"end to end: rb nucfreq -r chrS:1-{n} ({fmt}, {read_len}-base reads, {index})", "output_bytes": size, "md5": digest["device route"],
                           "rounds": a.rounds, "cpus": len(os.sched_getaffinity(0))}
                    for who, s in secs.items():
                        res[who] = {"seconds_median": round(float(np.median(s)), 4), "seconds_min": round(min(s), 4), "seconds_max": round(max(s), 4),
                                    "same_bytes": digest[who] == digest["device route"]}
                    if a.against:
                        o = res["the other build"]
                        spread = o["seconds_max"] - o["seconds_min"]
                        over = res["device route"]["seconds_median"] - o["seconds_median"]
                        res["pass_mark"] = {"device_route_median_minus_other_median": round(over, 4), "other_min_to_max_spread": round(spread, 4), "met": over <= spread}
                        passed.append(over <= spread)
                    print(json.dumps(res), flush=True)
                    assert len(set(digest.values())) == 1, "the routes printed other bytes"
                p = subprocess.run([rb, "nucfreq", "-r", f"chrS:1-{n}", "-s", bam], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                   env={**os.environ, **ienv, "RB_TIMING": "1", "RB_NUCFREQ_DEV_DECODE": "1"})
                print(json.dumps({"what": f"RB_TIMING laps, device route (--small, {read_len}-base reads, {index}, output to /dev/null)",
                                  "stderr": p.stderr.decode(errors="replace").splitlines()}), flush=True)
    if a.against:
        print(json.dumps({"what": "pass mark", "lines": len(passed), "met_on": sum(passed), "met_everywhere": all(passed)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--long-records", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--against", default=None, help="another build's rb to run alternately (its library beside it)")
    ap.add_argument("--tmp", default=None, help="where the BAMs and the outputs are written (default: the system's temporary directory)")
    a = ap.parse_args()
    if a.records or a.long_records:
        kernel(a)
    if a.e2e:
        end_to_end(a)


if __name__ == "__main__":
    main()
