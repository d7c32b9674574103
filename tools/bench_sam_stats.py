"""`rb stats` on SAM input: (a) rb_dev_parse_md and rb_dev_aln_stats (k_alnstats.hip) alone, (b) `rb stats in.sam` end to end.

  (a) kernels  --short N alignments with MD strings of tens of bytes, --long M strings of --long-bytes each (both built on the device from a
               tiled block, seeded), and a sweep of string lengths around the row / wave threshold (--sweep).  Each call is bracketed by HIP
               events on the engine's stream with its outputs allocated before: warmed, the median of --reps calls.  One JSON line per case:
               kernel_ms, the bytes the call has to move and the fraction of 8 TB/s they make.
                 rb_dev_parse_md   the MD bytes once + 16 B per record (its two offsets)
                 rb_dev_aln_stats  the row bytes in and out: 72 B reduce row + 16 B pos / flag / l_seq + 16 B MD counts + 2 B MD status /
                                   has_md in, 80 B out (the few ops it reads at both ends of a CIGAR are not counted)
               The threshold is a compile-time constant of the kernel (RB_MD_ROW_MAX).  To choose it, the sweep is run three times on one
               box: the product library, and the two variants `tools/mkvariant.sh md_rows --src k_alnstats.hip -DRB_MD_ROW_MAX=0xFFFFFFFFu`
               (every string a row) and `... md_waves ... -DRB_MD_ROW_MAX=0u` (every string the wavefront), selected with RB_VARIANT.
  (b) end to end  --e2e N alignments written as SAM, as a BAM twin at compression level 0 and as a PAF twin (seven-op CIGARs with M, as
               minimap2 writes them without --eqx, and an MD:Z: on every SAM / BAM record), then `rb stats` on each, --e2e-reps times, wall time of the process.  The
               parent commit cannot read SAM: its yardsticks are the BAM and the PAF line.

No oracle here: parity is the business of tests/test_gpu_aln_stats.py and tests/test_gpu_cli_stats_sam.py; the runs report the lines each route printed and how many strings were unusual.

  python tools/bench_sam_stats.py [--short 10000000] [--long 10000] [--long-bytes 1048576] [--sweep] [--e2e 200000] [--reps 20]
"""
import argparse
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


def md_block(n_bytes, seed):
    """MD-like text: numbers of one to four digits, single mismatches, short deletions"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n_bytes:
        out += b"%d" % int(rng.choice([0, 3, 17, 250, 4096]))
        k = 1 if rng.random() < .7 else int(rng.integers(2, 7))
        out += (b"" if k == 1 else b"^") + bytes(rng.choice(list(b"ACGT"), k - (k > 1)).astype(np.uint8))
    out = bytes(out[:n_bytes])
    return out[:-1] + b"0" if out.endswith(b"^") else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short", type=int, default=10_000_000)
    ap.add_argument("--long", type=int, default=10_000)
    ap.add_argument("--long-bytes", type=int, default=1 << 20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-bytes", type=int, default=1 << 30, help="text bytes per sweep point")
    ap.add_argument("--e2e", type=int, default=200_000)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tmp", default=None, help="where the end-to-end inputs are written (default: the system's temporary directory)")
    a = ap.parse_args()
    if a.short or a.long or a.sweep:
        kernels(a)
    if a.e2e:
        end_to_end(a)


def kernels(a):
    import torch
    import rustybam_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    shape = rustybam_amd.md_shape()
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

    def tiled_strings(block_strs, n):
        """n strings on the device, the block's strings over and over, each starting where the one before ended -> (text, off, end, bytes)"""
        blk = b"".join(block_strs)
        lens = np.array([len(s) for s in block_strs], np.int64)
        reps = -(-n // len(block_strs))
        text = torch.from_numpy(np.frombuffer(blk, np.uint8).copy()).to(dev).repeat(reps)
        text = torch.cat([text, torch.zeros(64, dtype=torch.uint8, device=dev)])
        ends = torch.from_numpy(np.cumsum(lens)).to(dev)
        end = (ends[None, :] + (torch.arange(reps, device=dev, dtype=torch.int64) * len(blk))[:, None]).reshape(-1)[:n].contiguous()
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), end[:-1]])
        return text, off, end, int(end[-1].item())

    def bench_md(what, text, off, end, n, n_bytes):
        out = torch.empty(4 * n + 4, dtype=torch.int32, device=dev)
        status = torch.empty(n + 1, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: eng.dev_parse_md(text.data_ptr(), off.data_ptr(), end.data_ptr(), n, out.data_ptr(), status.data_ptr()))
        moved = n_bytes + 16 * n
        print(json.dumps({"what": what, "library": variant, "shape": shape, "strings": n, "md_bytes": n_bytes, "bytes_per_string": round(n_bytes / n, 1),
                          "unusual": int((status[:n] != 0).sum().item()), "reps": a.reps, "kernel_ms": round(med, 4), "kernel_ms_min": round(lo, 4),
                          "kernel_ms_max": round(hi, 4), "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}), flush=True)
        return out, status

    # ---- (a) rb_dev_parse_md ----
    rng = np.random.default_rng(11)
    if a.short:
        block = [md_block(int(rng.integers(20, 60)), 100 + i) for i in range(4096)]
        text, off, end, nb = tiled_strings(block, a.short)
        md_out, md_status = bench_md("rb_dev_parse_md, short strings (tens of bytes)", text, off, end, a.short, nb)
        # ---- rb_dev_aln_stats on as many short-read alignments: clipped, an M op, the MD of above ----
        n = a.short
        cig = np.array([(5 << 4) | 4, (30 << 4) | 0, (2 << 4) | 1, (40 << 4) | 0, (3 << 4) | 2, (20 << 4) | 0, (4 << 4) | 4], np.uint32)
        ops = torch.from_numpy(cig.astype(np.int32)).to(dev).repeat(n)
        ops = torch.cat([ops, torch.zeros(64, dtype=torch.int32, device=dev)])
        op_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * len(cig)
        z = torch.zeros(n, dtype=torch.int64, device=dev)
        strand = torch.full((n,), ord("+"), dtype=torch.uint8, device=dev)
        view = eng.batch_view(n, n * len(cig), ops.data_ptr(), op_off.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), strand.data_ptr(), 0)
        red = torch.empty(n * 72 + 72, dtype=torch.uint8, device=dev)
        eng.dev_scan_records(view, red.data_ptr(), 0)
        pos = torch.arange(n, dtype=torch.int64, device=dev) * 7
        flag = ((torch.arange(n, device=dev) % 2) * 16).to(torch.int32)
        l_seq = torch.full((n,), 101, dtype=torch.int32, device=dev)
        has_md = torch.ones(n, dtype=torch.uint8, device=dev)
        rows = torch.empty(n * 80 + 80, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: eng.dev_aln_stats(view, red.data_ptr(), pos.data_ptr(), flag.data_ptr(), l_seq.data_ptr(), md_out.data_ptr(),
                                                      md_status.data_ptr(), has_md.data_ptr(), rows.data_ptr()))
        st = rows[: n * 80].view(torch.int32).view(n, 20)[:, 18]
        moved = (72 + 16 + 16 + 2 + 80) * n
        print(json.dumps({"what": "rb_dev_aln_stats, 7-op CIGARs with an MD", "library": variant, "alignments": n,
                          "rows_md_assert": int((st == rustybam_amd.ALN_PANIC_MD_ASSERT).sum().item()), "rows_ok": int((st == 0).sum().item()),
                          "reps": a.reps, "kernel_ms": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                          "algorithmic_bytes": moved, "fraction_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}), flush=True)
        del text, off, end, md_out, md_status, ops, op_off, z, strand, red, pos, flag, l_seq, has_md, rows
        torch.cuda.empty_cache()
    if a.long:
        text, off, end, nb = tiled_strings([md_block(a.long_bytes, 7)], a.long)
        bench_md(f"rb_dev_parse_md, long strings ({a.long_bytes} bytes)", text, off, end, a.long, nb)
        del text, off, end
        torch.cuda.empty_cache()
    if a.sweep:
        for ln in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 65536):
            n = max(a.sweep_bytes // ln, 256)
            text, off, end, nb = tiled_strings([md_block(ln, 1000 + ln + i) for i in range(16)], n)
            bench_md(f"sweep: strings of {ln} bytes", text, off, end, n, nb)
            del text, off, end
            torch.cuda.empty_cache()
    eng.close()


def end_to_end(a):
    """(b) rb stats in.sam, beside the BAM (compression level 0) and PAF twins of the same alignments"""
    import gzip
    import struct
    rb = os.path.join(ROOT, "rustybam_amd", "rb")
    rng = np.random.default_rng(5)
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        sam, bam, paf = (os.path.join(d, "in." + x) for x in ("sam", "bam", "paf"))
        refs = [("chr1", 250_000_000)]
        with open(sam, "wb") as fs, gzip.open(bam, "wb", compresslevel=0) as fb, open(paf, "wb") as fp:
            fs.write(b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:250000000\n")
            hdr = b"@HD\tVN:1.6\n"
            fb.write(b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", refs[0][1]))
            for i in range(a.e2e):
                m1, m2, m3 = (int(x) for x in rng.integers(20, 60, 3))
                cg = [(5, "S"), (m1, "M"), (2, "I"), (m2, "M"), (3, "D"), (m3, "M"), (4, "S")]
                md = b"%dA%d^ACG%dT%d" % (m1 - 1, m2, m3 // 2, m3 - m3 // 2 - 1)
                l_seq, pos, flag = 9 + m1 + 2 + m2 + m3, 1000 + 37 * i, 16 * (i & 1)
                name = b"read%d" % i
                cgt = b"".join(b"%d%s" % (n, c.encode()) for n, c in cg)
                fs.write(b"\t".join([name, b"%d" % flag, b"chr1", b"%d" % (pos + 1), b"60", cgt, b"*", b"0", b"0", b"N" * l_seq, b"*", b"MD:Z:" + md]) + b"\n")
                body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 0, len(cg), flag, l_seq, -1, -1, 0) + name + b"\0"
                body += b"".join(struct.pack("<I", (n << 4) | "MIDNSHP=X".index(c)) for n, c in cg) + b"\xff" * ((l_seq + 1) // 2) + b"\xff" * l_seq
                body += b"MDZ" + md + b"\0"
                fb.write(struct.pack("<i", len(body)) + body)
                t_en, q_en = pos + m1 + m2 + 3 + m3, 5 + m1 + 2 + m2 + m3
                fp.write(b"\t".join([name, b"%d" % l_seq, b"5", b"%d" % q_en, b"-" if flag else b"+", b"chr1", b"250000000", b"%d" % pos, b"%d" % t_en,
                                     b"0", b"0", b"60", b"cg:Z:%dM2I%dM3D%dM" % (m1, m2, m3)]) + b"\n")
        for what, args in (("rb stats in.sam", ["stats", sam]), ("rb stats in.sam (RB_GENERAL_PATH=1)", ["stats", sam]),
                           ("rb stats in.bam (level 0)", ["stats", bam]), ("rb stats --paf in.paf", ["stats", "--paf", paf])):
            env = dict(os.environ, RB_GENERAL_PATH="1") if "GENERAL" in what else dict(os.environ)
            env.pop("RB_VARIANT", None)
            secs, lines = [], None
            for _ in range(1 + a.e2e_reps):
                t0 = time.perf_counter()
                r = subprocess.run([rb, *args], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env)
                secs.append(time.perf_counter() - t0)
                assert r.returncode == 0, what
                lines = r.stdout.count(b"\n")
            print(json.dumps({"what": what, "alignments": a.e2e, "input_bytes": os.path.getsize(args[-1]), "lines": lines, "runs": a.e2e_reps,
                              "wall_s_median": round(float(np.median(secs[1:])), 4), "wall_s_min": round(min(secs[1:]), 4), "wall_s_first": round(secs[0], 4)}), flush=True)


if __name__ == "__main__":
    main()
