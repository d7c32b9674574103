"""`rb stats` on BAM input: (a) rb_dev_bam_records (k_bam.hip) alone, (b) `rb stats in.bam` end to end.

  (a) kernels  --short N short-read records (1 to 5 ops, an MD of 5 to 20 bytes, 150 bases of SEQ and QUAL, an NM:i in front of the MD) and
               --long M long-read records (about 3000 ops, an MD of about 8 KB, 15 kb of SEQ and QUAL), both built on the device by tiling a
               block of distinct records, and with --sweep a sweep of aux-area lengths around the row / wave threshold.  Each call is
               bracketed by HIP events on the engine's stream with its outputs allocated before: warmed, the median of --reps calls with
               min and max.  One JSON line per case: kernel_ms, the ALGORITHMIC bytes of the call and the fraction of 8 TB/s they make:
                 per record 36 B of fixed fields + the name + the aux bytes, read once;  4 B per op read + 4 B per op written;
                 46 B of output columns (tid, pos, flag, l_seq, has_md, md_off, md_end, op_off, status).  SEQ and QUAL do not count.
               The threshold is a compile-time constant of the kernel (RB_BAM_AUX_ROW_MAX).  To choose it, the sweep is run three times on one
               box: the product library, and the two variants `tools/mkvariant.sh bam_rows --src k_bam.hip -DRB_BAM_AUX_ROW_MAX=0xFFFFFFFFu`
               (every record a row) and `... bam_waves ... -DRB_BAM_AUX_ROW_MAX=0u` (every record the wavefront), selected with RB_VARIANT.
  (b) end to end  --e2e N[,N..] alignments (seven-op CIGARs with M, an MD:Z: on every record, every 50th record unmapped) written as BAM at
               compression level 0 (one gzip member) and as BGZF at level 1, then `rb stats` on each by the device route, by the record route
               (RB_GENERAL_PATH=1) and -- with --against RB, another build's `rb` with its library beside it, e.g. the parent commit's --
               by that build, alternately: one first run each, then --rounds rounds, medians with min and max, the outputs compared byte
               for byte.  The RB_TIMING laps of one more run of the device route are printed.

No oracle here: parity is the business of tests/test_gpu_bam_records.py and tests/test_gpu_cli_stats_bam.py.

  python tools/bench_bam_stats.py [--short 10000000] [--long 100000] [--sweep] [--reps 20] [--e2e 200000,2000000] [--rounds 5] [--against RB]
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PEAK = 8e12


def md_block(n_bytes, rng):
    """MD-like text: numbers of one to four digits, single mismatches, short deletions"""
    out = bytearray()
    while len(out) < n_bytes:
        out += b"%d" % int(rng.choice([0, 3, 17, 250, 4096]))
        k = 1 if rng.random() < .7 else int(rng.integers(2, 7))
        out += (b"" if k == 1 else b"^") + bytes(rng.choice(list(b"ACGT"), k - (k > 1)).astype(np.uint8))
    out = bytes(out[:n_bytes])
    return out[:-1] + b"0" if out.endswith(b"^") else out


def record(name, pos, flag, words, l_seq, aux):
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 0, len(words), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += struct.pack(f"<{len(words)}I", *words) + b"\xff" * ((l_seq + 1) // 2) + b"\xff" * l_seq + aux
    return struct.pack("<i", len(body)) + body


def block_of(kind, rng, aux_bytes=None):
    """-> (bytes of a block of distinct records, rec_off, rec_len within it, algorithmic bytes of the block, ops of the block)"""
    out, off, ln, alg, n_ops = bytearray(), [], [], 0, 0
    for i in range(4096 if kind == "short" else 16):
        if kind == "short":
            nc, l_seq, md_n = int(rng.integers(1, 6)), 150, int(rng.integers(5, 21))
        elif kind == "long":
            nc, l_seq, md_n = int(rng.integers(2800, 3200)), 15000, int(rng.integers(7800, 8200))
        else:  # the sweep: an aux area of aux_bytes, nearly all of it the MD
            nc, l_seq, md_n = 4, 150, aux_bytes - 11
        words = [(int(x) << 4) | int(o) for x, o in zip(rng.integers(1, 60, nc), rng.choice([0, 1, 0, 2, 0, 7, 8], nc))]
        name = b"read%d" % int(rng.integers(0, 10**int(rng.integers(1, 9))))
        aux = b"NMi" + struct.pack("<i", 3) + b"MDZ" + md_block(md_n, rng) + b"\0"
        r = record(name, 1000 + 37 * i, 16 * (i & 1), words, l_seq, aux)
        off.append(len(out) + 4)
        ln.append(len(r) - 4)
        out += r
        alg += 36 + len(name) + 1 + len(aux) + 8 * nc + 46
        n_ops += nc
    return bytes(out), np.array(off, np.int64), np.array(ln, np.int32), alg, n_ops


def kernels(a):
    import torch
    import rustybam_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    shape = rustybam_amd.bam_shape()
    variant = os.environ.get("RB_VARIANT", "product")

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
        return float(np.median(ms)), min(ms), max(ms)

    def bench(what, kind, n, aux_bytes=None):
        blk, boff, bln, balg, bops = block_of(kind, np.random.default_rng(11), aux_bytes)
        blk += b"\0" * (-len(blk) % 16)  # (whole blocks: every tile starts on a 16-byte boundary, the header's place in a real stream is not modelled)
        k = len(boff)
        reps = -(-n // k)
        n = reps * k
        data = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).to(dev).repeat(reps)
        data = torch.cat([data, torch.zeros(64, dtype=torch.uint8, device=dev)])
        base = (torch.arange(reps, device=dev, dtype=torch.int64) * len(blk))[:, None]
        rec_off = (torch.from_numpy(boff).to(dev)[None, :] + base).reshape(-1).contiguous()
        rec_len = torch.from_numpy(bln).to(dev).repeat(reps)
        total_ops = bops * reps
        i32 = lambda m: torch.empty(m + 4, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda m: torch.empty(m + 4, dtype=torch.int64, device=dev)  # noqa: E731
        u8 = lambda m: torch.empty(m + 64, dtype=torch.uint8, device=dev)  # noqa: E731
        tid, pos, flag, l_seq, has_md, md_off, md_end, op_off, status = i32(n), i64(n), i32(n), i32(n), u8(n), i64(n), i64(n), i64(n + 1), u8(n)
        ops = i32(total_ops + 64)
        scratch = u8(eng.bam_scratch_bytes(n))
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: eng.dev_bam_records(data.data_ptr(), rec_off.data_ptr(), rec_len.data_ptr(), n, tid.data_ptr(), pos.data_ptr(), flag.data_ptr(),
                                                        l_seq.data_ptr(), has_md.data_ptr(), md_off.data_ptr(), md_end.data_ptr(), op_off.data_ptr(),
                                                        ops.data_ptr(), total_ops, status.data_ptr(), scratch.data_ptr()))
        assert int(op_off[n].item()) == total_ops and int(status[:n].max().item()) == 0 and int(has_md[:n].min().item()) == 1
        moved = balg * reps
        print(json.dumps({"what": what, "library": variant, "shape": shape, "records": n, "ops": total_ops, "stream_bytes": len(blk) * reps,
                          "aux_bytes_per_record": aux_bytes, "reps": a.reps, "kernel_ms": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                          "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}), flush=True)
        del data, rec_off, rec_len, tid, pos, flag, l_seq, has_md, md_off, md_end, op_off, status, ops, scratch
        torch.cuda.empty_cache()

    if a.short:
        bench("rb_dev_bam_records, short reads (1-5 ops, MD of 5-20 bytes, 150 bases)", "short", a.short)
    if a.long:
        bench("rb_dev_bam_records, long reads (~3000 ops, MD of ~8 KB, 15 kb)", "long", a.long)
    if a.sweep:
        for aux in (64, 256, 512, 1024, 2048, 4096, 8192, 16384, 65536):
            bench(f"sweep: aux areas of {aux} bytes", "sweep", max(a.sweep_bytes // aux, 1024), aux)
    eng.close()


def bgzf(data, level=1, size=0xFF00):
    out = bytearray()
    for at in list(range(0, len(data), size)) + [len(data)]:
        chunk = data[at:at + size] if at < len(data) else b""
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        out += struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def md5(b):
    return hashlib.md5(b).hexdigest()


def end_to_end(a):
    rb = os.path.join(ROOT, "rustybam_amd", "rb")
    for n in [int(x) for x in a.e2e.split(",")]:
        rng = np.random.default_rng(5)
        hdr = b"@HD\tVN:1.6\n"
        out = bytearray(b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 250_000_000))
        m = rng.integers(20, 60, (n, 3))
        for i in range(n):
            m1, m2, m3 = (int(x) for x in m[i])
            words = [(5 << 4) | 4, (m1 << 4), (2 << 4) | 1, (m2 << 4), (3 << 4) | 2, (m3 << 4), (4 << 4) | 4]
            mdv = b"%dA%d^ACG%dT%d" % (m1 - 1, m2, m3 // 2, m3 - m3 // 2 - 1)
            out += record(b"read%d" % i, 1000 + 37 * i, (16 * (i & 1)) | (4 if i % 50 == 49 else 0), words, 9 + m1 + 2 + m2 + m3, b"NMi" + struct.pack("<i", 3) + b"MDZ" + mdv + b"\0")
        out = bytes(out)
        with tempfile.TemporaryDirectory(dir=a.tmp) as d:
            files = {"level 0": os.path.join(d, "l0.bam"), "BGZF level 1": os.path.join(d, "bgzf1.bam")}
            co = zlib.compressobj(0, zlib.DEFLATED, 31)
            open(files["level 0"], "wb").write(co.compress(out) + co.flush())
            open(files["BGZF level 1"], "wb").write(bgzf(out))
            for how, path in files.items():
                routes = [("device route", rb, {}), ("record route (RB_GENERAL_PATH=1)", rb, {"RB_GENERAL_PATH": "1"})]
                if a.against:
                    routes.append(("the other build", a.against, {}))
                secs, outs = {r[0]: [] for r in routes}, {}
                for i in range(1 + a.rounds):  # the first round warms the page cache and the device
                    for who, exe, env in routes:
                        e = {**os.environ, **env}
                        e.pop("RB_VARIANT", None)
                        t0 = time.perf_counter()
                        r = subprocess.run([exe, "stats", path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=e)
                        dt = time.perf_counter() - t0
                        assert r.returncode == 0, who
                        outs[who] = r.stdout
                        if i:
                            secs[who].append(dt)
                res = {"what": f"end to end: rb stats in.bam ({how})", "alignments": n, "input_bytes": os.path.getsize(path), "stream_bytes": len(out),
                       "lines": outs["device route"].count(b"\n"), "md5": md5(outs["device route"]), "rounds": a.rounds}
                for who in secs:
                    s = secs[who]
                    res[who] = {"seconds_median": round(float(np.median(s)), 4), "seconds_min": round(min(s), 4), "seconds_max": round(max(s), 4),
                                "same_bytes": outs[who] == outs["device route"]}
                if a.against:
                    o = res["the other build"]
                    spread = o["seconds_max"] - o["seconds_min"]
                    res["pass_mark"] = {"device_median_minus_other_median": round(res["device route"]["seconds_median"] - o["seconds_median"], 4),
                                        "other_min_to_max_spread": round(spread, 4),
                                        "met": res["device route"]["seconds_median"] <= o["seconds_median"] + spread}
                print(json.dumps(res), flush=True)
                p = subprocess.run([rb, "stats", path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env={**os.environ, "RB_TIMING": "1"})
                print(json.dumps({"what": f"RB_TIMING laps, device route ({how}, {n} alignments)", "stderr": p.stderr.decode(errors="replace").splitlines()}), flush=True)
                assert all(v == outs["device route"] for v in outs.values()), "the routes printed other bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short", type=int, default=10_000_000)
    ap.add_argument("--long", type=int, default=100_000)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-bytes", type=int, default=1 << 30, help="aux bytes per sweep point")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", default="200000,2000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--against", default=None, help="another build's rb to run alternately (its library beside it)")
    ap.add_argument("--tmp", default=None, help="where the end-to-end inputs are written (default: the system's temporary directory)")
    a = ap.parse_args()
    if a.short or a.long or a.sweep:
        kernels(a)
    if a.e2e and a.e2e != "0":
        end_to_end(a)


if __name__ == "__main__":
    main()
