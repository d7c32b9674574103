"""`rb stats [--qbed] in.bam` through the device route (stats_bam_text: rb_dev_bam_records, rb_dev_scan_records, rb_dev_parse_md,
rb_dev_aln_stats) byte for byte against the oracle: stdout, the exit code, the panic's presence.  The three golden BAMs; the deep set
of tests/sam_deep_util.py (unmapped records in between) as plain gzip, as BGZF in blocks that records and fields straddle, and on
stdin; a file of CG long CIGARs; every panic variant that a BAM can carry and a record that does not fit its block, deep in the file;
files cut inside a record and inside a block_size; the record route (RB_GENERAL_PATH=1) beside it.  (The `cigar_text` variant is an edit
of a SAM line: a BAM cannot carry a malformed CIGAR text.)"""
import gzip
import os
import re
import struct
import subprocess

import pytest

import rustybam_amd
import bam_rec_util as B
import sam_deep_util as D
import sam_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
WARNING = "contains 'M'".encode()
QBED = [False, True]


def rb_stats(arg, qbed, env=None, stdin=None):
    """one start of `rb stats` -> (exit code, stdout, (records left to the host, records) / None, stderr)"""
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    r = subprocess.run([RB, "stats", *(["--qbed"] if qbed else []), str(arg)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env={**os.environ, "RB_TIMING": "1", **(env or {})}, timeout=120)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # nothing more is started on a card that faulted
        pytest.exit(f"rb stats {arg} ended with {r.returncode}: {r.stderr[-400:]!r}", returncode=3)
    m = re.search(rb"stats_bam_text: records left to the host (\d+) of (\d+)", r.stderr)
    assert (m is not None) == (b"rb_dev_bam_records" in r.stderr)
    return r.returncode, r.stdout, ((int(m.group(1)), int(m.group(2))) if m else None), r.stderr


def _oracle_both(oracle, path):
    return {q: oracle.cli("stats", *(["--qbed"] if q else []), path) for q in QBED}


def _gz(path, data):
    with gzip.open(path, "wb", compresslevel=1) as f:
        f.write(data)
    return path


def bgzf_of_single_bytes(data):
    """sam_util.bgzf_bytes(data, (1,)) without a deflate call per byte: the 256 possible blocks once"""
    table = [U.bgzf_bytes(bytes([x]), (1,)) for x in range(256)]
    eof = U.bgzf_bytes(b"", (1,))
    table = [t[:len(t) - len(eof)] for t in table]
    return b"".join(table[x] for x in data) + eof


@pytest.mark.parametrize("bam", ["asm_small.bam", "stats.bam", "test.bam"])
def test_golden_bams(oracle, golden, bam):
    path = os.path.join(golden, bam)
    n_rec = len(U.read_bam(path)[1])
    for qbed in QBED:
        want = oracle.cli("stats", *(["--qbed"] if qbed else []), path)
        rc, out, left, err = rb_stats(path, qbed)
        assert (rc, out) == want and rc == 0, err[-300:]
        assert left == (0, n_rec) and b"rb_dev_bam_records" in err
        rc, out, left, err = rb_stats(path, qbed, env={"RB_GENERAL_PATH": "1"})
        assert (rc, out) == want and left is None and b"rb_dev_bam_records" not in err


@pytest.fixture(scope="module")
def deep(oracle, tmp_path_factory):
    assert rustybam_amd.md_shape() == D.SHAPE, "the deep set is built for another shape of rb_k_parse_md"
    d = tmp_path_factory.mktemp("deep_bam")
    refs, recs = D.deep_set(D.SHAPE)
    assert 50 < sum(1 for r in recs if r["flag"] & 4) < len(recs) - D.N_MAPPED + 1
    data = U.bam_bytes(refs, recs)
    twin = _gz(d / "twin.bam", data)
    want = _oracle_both(oracle, twin)
    assert want[False][0] == 0 and want[False][1].count(b"\n") == 1 + D.N_MAPPED
    n_warn = sum(1 for r in D.mapped_of(recs) if U.span_model(r)["flags"] & U.ALN_WARN_M)
    return dict(dir=d, refs=refs, recs=recs, data=data, twin=twin, want=want, n_warn=n_warn)


WAYS = {"gzip": None, "bgzf_FF00": (0xFF00,), "bgzf_4096_37": (4096, 37), "bgzf_1": (1,), "stdin": "stdin", "stdin_bgzf": "stdin_bgzf"}


@pytest.fixture(scope="module")
def deep_files(deep):
    out = {}
    for way, sizes in WAYS.items():
        if way == "gzip":
            out[way] = deep["twin"]
        elif way.startswith("bgzf"):
            raw = bgzf_of_single_bytes(deep["data"]) if sizes == (1,) else U.bgzf_bytes(deep["data"], sizes)
            if sizes == (1,):
                assert raw[:200] == U.bgzf_bytes(deep["data"][:50], (1,))[:200] and raw.count(b"\x1f\x8b\x08\x04") >= len(deep["data"])
            out[way] = deep["dir"] / f"{way}.bam"
            out[way].write_bytes(raw)
    return out


@pytest.mark.parametrize("qbed", QBED)
@pytest.mark.parametrize("way", sorted(WAYS))
def test_the_deep_set_in_every_container(deep, deep_files, way, qbed):
    if way == "stdin":
        got = rb_stats("-", qbed, stdin=deep["twin"].read_bytes())
    elif way == "stdin_bgzf":
        got = rb_stats("-", qbed, stdin=deep_files["bgzf_4096_37"].read_bytes())
    else:
        got = rb_stats(deep_files[way], qbed)
    rc, out, left, err = got
    assert (rc, out) == deep["want"][qbed] and rc == 0, (way, rc, err[-300:])
    # the records left to the host are exactly the designed declines (a zero-padded MD number of ten digits), of all records of the file
    assert left == (D.N_DECLINES, len(deep["recs"])), (way, left)
    assert err.count(WARNING) == deep["n_warn"] > 40


@pytest.mark.parametrize("qbed", QBED)
def test_the_record_route_gives_the_same_bytes(deep, deep_files, qbed):
    rc, out, left, err = rb_stats(deep_files["bgzf_4096_37"], qbed, env={"RB_GENERAL_PATH": "1"})
    assert (rc, out) == deep["want"][qbed] and left is None and b"rb_dev_bam_records" not in err and err.count(WARNING) == deep["n_warn"]


def test_a_file_of_long_cigars(oracle, tmp_path):
    cases = [c for c in B.cg_cases() + B.aux_cases(rustybam_amd.bam_shape()[1])]
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    recs = B.records_of(data, off, ln, m, B.REFS)
    ill = ("unterminated", "overrun", "left_behind_3_is_a_head", "unknown_type", "md_as_H", "B_unknown_subtype")  # (the oracle reads past those)
    keep = [(lb, b) for (lb, b), r in zip(cases, recs) if not any(x in lb for x in ill) and U.stats_model(B.REFS, [r], False)[1] == 0]
    labels = [lb for lb, _ in keep]
    assert {"applies_3", "applies_65536", "applies_70000", "two_tags_the_last_wins", "behind_md", "tag_phase_7", "md_len_5000", "wave_two_mds"} <= set(labels)
    path = _gz(tmp_path / "cg.bam", B.stream([b for _, b in keep])[0])
    for qbed in QBED:
        want = oracle.cli("stats", *(["--qbed"] if qbed else []), path)
        assert want[0] == 0 and want[1].count(b"\n") == 1 + len(keep) - sum(1 for lb in labels if lb == "unmapped_with_tag")
        rc, out, left, err = rb_stats(path, qbed)
        assert (rc, out) == want and left == (0, len(keep)), err[-300:]
        assert rb_stats(path, qbed, env={"RB_GENERAL_PATH": "1"})[:2] == want


@pytest.fixture(scope="module")
def variants(oracle, deep):
    out = {}
    for name, v in D.panic_variants(D.SHAPE).items():
        if v["sam_edit"]:
            continue
        path = _gz(deep["dir"] / f"{name}.bam", U.bam_bytes(deep["refs"], v["recs"]))
        out[name] = dict(path=path, want=_oracle_both(oracle, path), index=v["index"], recs=v["recs"])
    # a record that does not fit its block, in front of mapped record 333: the same bytes with its l_seq field raised
    k = D.file_index(deep["recs"], 333)
    _, off, ln = B.hop(deep["data"])
    data = bytearray(deep["data"])
    struct.pack_into("<I", data, int(off[k]) + 16, int(ln[k]))
    path = _gz(deep["dir"] / "no_fit.bam", bytes(data))
    out["no_fit"] = dict(path=path, want=_oracle_both(oracle, path), index=333, recs=deep["recs"])
    return out


@pytest.mark.parametrize("name", sorted(set(D.PANIC_AT) - {"cigar_text"}) + ["no_fit"])
def test_a_panic_deep_in_the_file_leaves_the_lines_before_it(deep, variants, name):
    v = variants[name]
    k = v["index"]
    n_warn = sum(1 for r in D.mapped_of(v["recs"])[:k] if U.span_model(r)["flags"] & U.ALN_WARN_M)
    for qbed in QBED:
        rc, out, left, err = rb_stats(v["path"], qbed)
        assert (rc, out) == v["want"][qbed] and rc == 101 and out.count(b"\n") == 1 + k, (name, qbed, rc, out.count(b"\n"), err[-300:])
        assert deep["want"][qbed][1].startswith(out) and b"panicked" in err and err.count(WARNING) == n_warn
        g = rb_stats(v["path"], qbed, env={"RB_GENERAL_PATH": "1"})
        assert g[:2] == (rc, out) and g[3].count(WARNING) == n_warn
        if name == "no_fit":
            assert b"do not fit the block" in err and b"do not fit the block" in g[3]


@pytest.mark.parametrize("cut", ["inside_a_record", "inside_a_block_size", "behind_the_last_record"])
def test_a_file_that_ends_early(oracle, deep, tmp_path, cut):
    _, off, ln = B.hop(deep["data"])
    k = D.file_index(deep["recs"], 200)
    at = {"inside_a_record": int(off[k]) + 40, "inside_a_block_size": int(off[k]) - 2, "behind_the_last_record": len(deep["data"])}[cut]
    path = _gz(tmp_path / "cut.bam", deep["data"][:at])
    for qbed in QBED:
        want = oracle.cli("stats", *(["--qbed"] if qbed else []), path)
        rc, out, left, err = rb_stats(path, qbed)
        assert (rc, out) == want, (cut, rc, want[0], err[-300:])
        assert (rc == 101 and out.count(b"\n") == 1 + 200 and b"truncated BAM file" in err) if cut != "behind_the_last_record" else rc == 0
        assert rb_stats(path, qbed, env={"RB_GENERAL_PATH": "1"})[:2] == want
