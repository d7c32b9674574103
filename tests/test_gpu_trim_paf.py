"""trim-paf end to end against the oracle CLI's bytes on generated files (tests/trim_util.py): irregular CIGARs whose clips the serial pair
kernel moves behind the ops and later passes cut again, query groups deep enough for dozens of deferred passes, contained / identical /
touching spans, tied overlaps, q_st = 0 behind ops that consume no query, names whose byte order is not their numeric order.  Three
routes: `rb trim-paf`, trim_driver.ResidentTrim (the batch resident on the device), trim_driver.overlapping_paf_recs (host API)."""
import os
import subprocess

import numpy as np
import pytest

import rustybam_amd
from rustybam_amd import capi, trim_driver
from rbtest_util import compare_hits, recs_from_lines
from trim_util import CONFIGS, format_recs, format_resident, oracle_args, panic_group, parse, pipeline_file, rb_args, trim_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
SEED = 1


def _rb(args, stdin=None, env=None):
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    r = subprocess.run([RB, *map(str, args)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=None if env is None else {**os.environ, **env})
    return r.returncode, r.stdout


@pytest.fixture(scope="module")
def paf(oracle, tmp_path_factory):
    text = trim_file(SEED)
    path = tmp_path_factory.mktemp("trim") / "irregular.paf"
    path.write_bytes(text)
    return text, str(path)


def _resident(text, torch, dev, eng):
    r = recs_from_lines(text.decode().splitlines())
    rank = {q: i for i, q in enumerate(sorted(set(r.q_name)))}           # groups in the order of the names (the reference sorts by name)
    group = np.array([rank[q] for q in r.q_name])
    T = trim_driver.ResidentTrim(eng, torch, dev, r.ops, r.op_off, r.t_st, r.t_en, r.q_st, r.q_en, r.strand, group)
    return r, T


def test_rb_trim_paf_equals_the_oracle_on_irregular_deep_files(oracle, paf):
    """every configuration, from a file and from stdin; clips copied (RB_TRIM_COPY=1); two shards whose name ranges meet between two
    groups of one name prefix"""
    text, path = paf
    for cfg in CONFIGS:
        orc, want = oracle.cli(*oracle_args(cfg, path))
        assert orc == 0 and want.count(b"\n") > 300 and b"_TO." in want, cfg
        for src, stdin in ((path, None), ("-", text)):
            rc, got = _rb(rb_args(cfg, src), stdin=stdin)
            assert rc == 0 and got == want, (cfg, src)
    orc, want = oracle.cli(*oracle_args("default", path))
    rc, got = _rb(rb_args("default", path), env={"RB_TRIM_COPY": "1"})
    assert rc == 0 and got == want, "RB_TRIM_COPY=1"
    # --gpus 2 cuts the sorted query names into two ranges of about equal bytes: here both sides of the middle are 'q' names
    names = sorted({ln.split(b"\t")[0] for ln in text.splitlines()})
    weight = {q: 0 for q in names}
    for ln in text.splitlines():
        weight[ln.split(b"\t")[0]] += len(ln) + 1
    acc = np.cumsum([weight[q] for q in names])
    mid = int(np.searchsorted(acc, acc[-1] // 2))
    assert all(q.startswith(b"q") for q in names[max(0, mid - 3):mid + 4]), names[mid - 3:mid + 4]
    for cfg in ("default", "remove"):
        orc, want = oracle.cli(*oracle_args(cfg, path))
        rc, got = _rb(["--gpus", 2, *rb_args(cfg, path)], env={"RB_GPUS_SAME_DEVICE": "1"})
        assert rc == 0 and got == want, ("--gpus 2", cfg)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_resident_trim_equals_the_oracle_on_irregular_deep_files(oracle, paf, cfg):
    """trim_driver.ResidentTrim: the serial kernel cuts irregular records and copies their clips behind the ops in use; a later pass
    cuts such a MOVED record again from where it was moved to; gathered and printed, the bytes of the oracle CLI"""
    import torch
    text, path = paf
    c = CONFIGS[cfg]
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    r, T = _resident(text, torch, dev, eng)
    norm0 = T.d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)[:r.n].copy()
    off_at_start = T.op_off_host.copy()
    moved_cut_again = []

    def on_pass(i, k, d_l, d_r, d_rows):
        recs = np.r_[d_l[:k].cpu().numpy().view(np.uint32), d_r[:k].cpu().numpy().view(np.uint32)].astype(np.int64)
        if i > 0:
            moved_cut_again.extend(int(x) for x in recs[off_at_start[recs] >= T.n_ops0])
        off_at_start[:] = T.d_off[:r.n + 1].cpu().numpy().view(np.uint64)

    T.run(c["scores"], c["policy"], on_pass=on_pass)
    assert T.passes > 10 and T.pairs_by_wave < T.pairs_done, (T.passes, T.pairs_by_wave, T.pairs_done)
    assert moved_cut_again, "no pass cut a record an earlier pass had moved"
    d_new, new_off, norm = T.gather()
    got = format_resident(r, norm0, norm, d_new.cpu().numpy().view(np.uint32), new_off, T.order, keep=~T.contained if c["remove"] else None)
    orc, want = oracle.cli(*oracle_args(cfg, path))
    assert orc == 0 and got.encode() == want
    del d_new
    T.release()
    torch.cuda.synchronize()
    eng.close()


def test_host_driver_equals_the_oracle_on_irregular_deep_files(engine, oracle, paf):
    text, path = paf
    out = trim_driver.overlapping_paf_recs(engine, parse(text), (1, 1, 1), False, rustybam_amd.BSEARCH_MODERN)
    orc, want = oracle.cli(*oracle_args("default", path))
    assert orc == 0 and format_recs(out).encode() == want


def test_a_group_the_reference_panics_on(oracle, paf, tmp_path):
    """one group whose pair cut panics in the reference, among the generated ones: rb exits 101 and prints nothing, ResidentTrim raises"""
    import torch
    text, _ = paf
    bad = tmp_path / "panic.paf"
    bad.write_bytes(text + panic_group())
    assert oracle.cli(*oracle_args("default", str(bad)))[0] == 101
    for cfg in ("default", "legacy"):
        rc, out = _rb(rb_args(cfg, str(bad)))
        assert rc == 101 and out == b"", cfg
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    r, T = _resident(text + panic_group(), torch, dev, eng)
    with pytest.raises(RuntimeError, match="status 16"):
        T.run((1, 1, 1), rustybam_amd.BSEARCH_MODERN)
    T.release()
    torch.cuda.synchronize()
    eng.close()


def test_readme_pipeline_with_irregular_records(oracle, paf, tmp_path):
    """`rb trim-paf f | rb break-paf --max-size 100 -` against the oracle's trim-paf | break-paf: on the groups the oracle's pipeline
    takes, the same bytes; on the whole file, break-paf's panic (exit code 101) as in the oracle"""
    src = tmp_path / "pipeline.paf"
    src.write_bytes(pipeline_file(SEED))
    for path, want_rc in ((str(src), 0), (paf[1], 101)):
        p1 = subprocess.Popen([RB, "trim-paf", path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        p2 = subprocess.run([RB, "break-paf", "--max-size", "100", "-"], stdin=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        p1.stdout.close()
        assert p1.wait() == 0 and p2.returncode == want_rc, path
        orc, trimmed = oracle.cli("trim-paf", path)
        orc2, want = oracle.cli("break-paf", "--max-size", "100", "-", stdin=trimmed)
        assert (orc, orc2) == (0, want_rc), path
        if want_rc == 0:
            assert p2.stdout == want and want.count(b"\n") > trimmed.count(b"\n") > 200 and trimmed.count(b"_TO.") > 20
        else:  # (rb panics before it prints, as tests/test_gpu_cli.py holds it to for break-paf)
            assert p2.stdout == b""


def test_op_starts_refuses_a_batch_whose_records_a_pass_moved(oracle, paf):
    """RB_LIFT_OP_STARTS on a resident batch after passes that moved records (the serial kernel's clips lie behind batch->n_ops): both
    rb_dev_break and rb_dev_liftover refuse with RB_E_INVALID before any clip kernel runs.  The same engine then runs both on the
    gathered dense batch, equal to the oracle on those records."""
    import torch
    from devutil import DevBatch
    text, _ = paf
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    r, T = _resident(text, torch, dev, eng)
    T.run((1, 1, 1), rustybam_amd.BSEARCH_MODERN)
    assert T.pairs_by_wave < T.pairs_done
    with pytest.raises(ValueError):
        DevBatch.from_trimmed(torch, eng, dev, T)
    B = DevBatch.from_trimmed(torch, eng, dev, T, allow_moved=True)
    moved = np.flatnonzero(T.d_off[:r.n].cpu().numpy().view(np.uint64) >= T.n_ops0)
    assert len(moved) > 0
    w = (np.zeros(4, np.uint32), np.array([0, 1000, 20_000, 50_000], np.uint64), np.array([600, 9000, 40_000, 200_000], np.uint64))
    for kind, kw in (("break", dict(max_size=100)), ("liftover", dict(windows=w))):
        for extra in (rustybam_amd.BREAK_ONE_WALK, 0):
            with pytest.raises(capi.RbError, match=r"failed with -1: RB_LIFT_OP_STARTS: record \d+ lies outside"):
                B.run(policy=rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_OP_STARTS | extra, **kw)
    B.last = None
    torch.cuda.synchronize()
    d_new, new_off, norm = T.gather()
    contig = {q: i for i, q in enumerate(dict.fromkeys(r.t_name))}
    contig = np.array([contig[t] for t in r.t_name], np.uint32)
    d_c = [torch.from_numpy(np.ascontiguousarray(norm[k]).view(np.int64)).to(dev) for k in ("t_st", "t_en", "q_st", "q_en")]
    G = DevBatch.from_device(torch, eng, dev, d_new, int(new_off[-1]), new_off, d_c, torch.from_numpy(r.strand).to(dev))
    G.contig_host = contig
    G.d_contig.copy_(torch.from_numpy(contig.view(np.int32)).to(dev))
    ops = d_new[:int(new_off[-1])].cpu().numpy().view(np.uint32).copy()
    ob = oracle.Batch(ops, new_off, norm["t_st"], norm["t_en"], norm["q_st"], norm["q_en"], r.strand, contig)
    rows, out, cnt = G.run(None, max_size=100)
    assert not cnt["overflow"]
    hr, hout = G.host_rows(rows, out)
    orows, oout = oracle.break_paf(ob, 100)
    compare_hits(hr, hout, orows, oout, "break-paf on the gathered batch")
    wc = np.repeat(np.arange(len(set(r.t_name)), dtype=np.uint32), 4)
    ws = np.tile(w[1], len(set(r.t_name)))
    we = np.tile(w[2], len(set(r.t_name)))
    rows, out, cnt = G.run((wc, ws, we))
    assert not cnt["overflow"]
    hr, hout = G.host_rows(rows, out)
    orows, oout = oracle.liftover(ob, wc, ws, we)
    assert len(orows) > 50
    compare_hits(hr, hout, orows, oout, "liftover on the gathered batch")
    del B, G, rows, out, d_new
    T.release()
    torch.cuda.synchronize()
    eng.close()
