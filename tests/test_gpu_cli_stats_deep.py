"""`rb stats [--qbed]` on the deep record set of tests/sam_deep_util.py (test_sam_deep_inputs.py holds the set and the models to the oracle):
hundreds of records in three blocks of rb_k_aln_stats, MD strings in the wavefront form of rb_k_parse_md, unmapped records in between,
designed declines in every block, panics deep in the file.  The yardstick is always the oracle on the BAM twin -- never `rb` -- and every
comparison is byte for byte: stdout and the exit code.  The SAM goes in as a file, on stdin, gzipped (one member and several) and through
the record route (RB_GENERAL_PATH=1); the BAM twin itself goes through `rb stats` too, whose route shares the span rules."""
import gzip
import os
import re
import subprocess

import pytest

import rustybam_amd
import sam_deep_util as D
import sam_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
ROUTES = ["file", "stdin", "gz", "general", "bam"]
WARNING = "contains 'M'".encode()


def rb_stats(arg, qbed, env=None, stdin=None):
    """one start of `rb stats` -> (exit code, stdout, records left to the host / None, stderr)"""
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    r = subprocess.run([RB, "stats", *(["--qbed"] if qbed else []), str(arg)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env={**os.environ, "RB_TIMING": "1", **(env or {})}, timeout=120)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # nothing more is started on a card that faulted
        pytest.exit(f"rb stats {arg} ended with {r.returncode}: {r.stderr[-400:]!r}", returncode=3)
    m = re.search(rb"stats_sam_text: records left to the host (\d+) of (\d+)", r.stderr)
    return r.returncode, r.stdout, (int(m.group(1)) if m else None), r.stderr


def run_route(route, sam, bam, tmp_path, qbed):
    if route == "bam":
        got = rb_stats(bam, qbed)
    elif route == "stdin":
        got = rb_stats("-", qbed, stdin=sam)
    else:
        path = tmp_path / ("in.sam.gz" if route == "gz" else "in.sam")
        if route == "gz":
            with gzip.open(path, "wb", compresslevel=1) as f:
                f.write(sam)
        else:
            path.write_bytes(sam)
        got = rb_stats(path, qbed, env={"RB_GENERAL_PATH": "1"} if route == "general" else None)
    assert (b"stats_sam_text" in got[3]) == (route in ("file", "stdin", "gz")), got[3][-400:]  # the timing output names the device entry point
    return got


def _oracle_both(oracle, bam):
    return {q: oracle.cli("stats", *(["--qbed"] if q else []), bam) for q in (False, True)}


@pytest.fixture(scope="module")
def deep(oracle, tmp_path_factory):
    """the main set once: refs, recs, SAM text, the BAM twin's path, the oracle's (exit code, stdout) on it by qbed, the model's warnings"""
    assert rustybam_amd.md_shape() == D.SHAPE, "the deep set is built for another shape of rb_k_parse_md"
    d = tmp_path_factory.mktemp("deep")
    refs, recs = D.deep_set(D.SHAPE)
    bam = d / "twin.bam"
    U.write_bam(bam, refs, recs)
    want = _oracle_both(oracle, bam)
    assert want[False][0] == 0 and want[False][1].count(b"\n") == 1 + D.N_MAPPED
    n_warn = sum(1 for r in D.mapped_of(recs) if U.span_model(r)["flags"] & U.ALN_WARN_M)
    return dict(refs=refs, recs=recs, sam=U.sam_text(refs, recs), bam=bam, want=want, n_warn=n_warn)


@pytest.fixture(scope="module")
def variants(oracle, deep, tmp_path_factory):
    """name -> dict(sam, bam (None: the SAM line edit), want by qbed, index)"""
    d = tmp_path_factory.mktemp("variants")
    out = {}
    for name, v in D.panic_variants(D.SHAPE).items():
        sam = D.variant_sam(deep["refs"], v)
        if v["sam_edit"]:  # the oracle's lines in front of the edited line: those of the main set
            bam = None
            want = {q: (101, b"".join(deep["want"][q][1].splitlines(True)[:1 + v["index"]])) for q in (False, True)}
        else:
            bam = d / f"{name}.bam"
            U.write_bam(bam, deep["refs"], v["recs"])
            want = _oracle_both(oracle, bam)
        out[name] = dict(sam=sam, bam=bam, want=want, index=v["index"], recs=v["recs"])
    return out


@pytest.mark.parametrize("qbed", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_the_deep_set_equals_the_oracle_on_the_bam_twin(deep, tmp_path, route, qbed):
    rc, out, left, err = run_route(route, deep["sam"], deep["bam"], tmp_path, qbed)
    assert (rc, out) == deep["want"][qbed] and rc == 0, (route, qbed, rc, err[-300:])
    assert left == (D.N_DECLINES if route in ("file", "stdin", "gz") else None), (route, left)
    # M without MD: the reference warns once per such record (bamstats.rs:145-153); no designed decline is one (each has an MD)
    assert err.count(WARNING) == deep["n_warn"] > 40, (route, err.count(WARNING), deep["n_warn"])


def _members(text, cuts):
    """the text as gzip members cut at the offsets"""
    edges = [0] + sorted(cuts) + [len(text)]
    return b"".join(gzip.compress(text[a:b], compresslevel=1) for a, b in zip(edges, edges[1:]))


@pytest.mark.parametrize("qbed", [False, True])
def test_a_gzip_file_of_several_members(deep, tmp_path, qbed):
    """cut in the middle of a line, in the middle of an MD string (a short one and one in the wavefront form), and into an empty member"""
    sam, off, end = D.sam_with_md_extents(deep["refs"], deep["recs"])
    assert sam == deep["sam"]
    long_k = next(k for k in range(300, len(off)) if int(end[k]) - int(off[k]) > D.SHAPE[1])
    short_k = next(k for k in range(len(off)) if 0 < int(end[k]) - int(off[k]) < 64)
    name_at = sam.index(b"\nbulk_200\t") + 5
    cuts = [name_at, int(off[short_k]) + 3, (int(off[long_k]) + int(end[long_k])) // 2, int(end[-1]) - 1, int(end[-1]) - 1]
    path = tmp_path / "members.sam.gz"
    path.write_bytes(_members(sam, cuts))
    assert gzip.decompress(path.read_bytes()) == sam and path.read_bytes().count(b"\x1f\x8b\x08") >= 6
    rc, out, left, err = rb_stats(path, qbed)
    assert (rc, out) == deep["want"][qbed] and left == D.N_DECLINES, err[-300:]


@pytest.mark.parametrize("qbed", [False, True])
@pytest.mark.parametrize("what", ["sam", "bam"])
def test_bgzf_blocks_of_irregular_sizes(deep, tmp_path, what, qbed):
    """the SAM text as .sam.bgz and the BAM twin as a real BGZF file (the twin the oracle reads is one plain gzip member): blocks of 1 to
    65280 bytes, lines, records and MD strings straddling them, the empty end-of-file block"""
    path = tmp_path / ("in.sam.bgz" if what == "sam" else "in.bam")
    path.write_bytes(U.bgzf_bytes(deep["sam"] if what == "sam" else U.bam_bytes(deep["refs"], deep["recs"]), D.BGZF_SIZES))
    rc, out, left, err = rb_stats(path, qbed)
    assert (rc, out) == deep["want"][qbed], (what, rc, err[-300:])
    assert left == (D.N_DECLINES if what == "sam" else None) and err.count(WARNING) == deep["n_warn"]


LAYOUTS = {  # name -> (what layout_sam makes of the set, --qbed)
    "no_newline_at_the_end": (dict(last="nothing"), False),
    "an_empty_last_line": (dict(last="empty"), True),
    "md_ends_the_text": (dict(md_place="last", last="nothing"), True),
    "md_first": (dict(md_place="first"), False),
    "md_in_the_middle": (dict(md_place="middle"), True),
    "md_last": (dict(md_place="last"), False),
    "md_in_turn_and_a_second_md": (dict(md_place="cycle", second_md=True), False),
    "a_second_md_at_the_end_of_the_text": (dict(md_place="first", second_md=True, last="nothing"), True),
}


@pytest.mark.parametrize("route", ["file", "general"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_line_layouts(deep, tmp_path, layout, route):
    """where the MD tag stands among the optional fields and how the text ends changes nothing; of two MD:Z: on a line the first counts
    (the BAM twin carries the first)"""
    kw, qbed = LAYOUTS[layout]
    sam = D.layout_sam(deep["refs"], deep["recs"], **kw)
    assert sam != deep["sam"]
    rc, out, left, err = run_route(route, sam, None, tmp_path, qbed)
    assert (rc, out) == deep["want"][qbed], (layout, route, rc, err[-300:])
    assert left == (D.N_DECLINES if route == "file" else None) and err.count(WARNING) == deep["n_warn"]


# (a BAM cannot carry a malformed CIGAR text: the line edit has no twin to run)
@pytest.mark.parametrize("name,route", [(n, r) for n in sorted(D.PANIC_AT) for r in ("file", "general", "bam") if (n, r) != ("cigar_text", "bam")])
def test_a_panic_deep_in_the_file_leaves_the_lines_before_it(deep, variants, tmp_path, name, route):
    v = variants[name]
    k = v["index"]
    # the reference takes the records one after the other and warns behind read_pos (bamstats.rs:190-197, then :145-153): once for every
    # M-without-MD record in front of the panic, not for the record that panics, not for any behind it
    n_warn = sum(1 for r in D.mapped_of(v["recs"])[:k] if U.span_model(r)["flags"] & U.ALN_WARN_M)
    assert 0 < n_warn < deep["n_warn"]
    for qbed in (False, True):
        rc, out, left, err = run_route(route, v["sam"], v["bam"], tmp_path, qbed)
        assert (rc, out) == v["want"][qbed] and rc == 101 and out.count(b"\n") == 1 + k, (name, route, qbed, rc, out.count(b"\n"), err[-300:])
        assert deep["want"][qbed][1].startswith(out) and b"panicked" in err
        assert err.count(WARNING) == n_warn, (name, route, qbed, err.count(WARNING), n_warn)
        if name == "cigar_text":
            line = 1 + len(deep["refs"]) + D.file_index(v["recs"], k) + 1
            assert b"line %d:" % line in err, err[-300:]
            if route == "file":  # the list ends in front of the line: the declines behind it are never looked at
                assert left == sum(1 for d in D.DECLINE_AT if d < k)
        elif route == "file":  # (a decline that is a panic is the device's to report: a hard clip comes first)
            assert left == D.N_DECLINES
