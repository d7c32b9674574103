"""The generator of trim-paf inputs (tests/trim_util.py) stays hard: the files the GPU tests use hold what the composition of trim-paf's
device steps gets wrong most easily, the oracle accepts every one of them, and the host driver's bookkeeping on the oracle's own kernels
prints the oracle CLI's bytes (so a difference on the device is the device's)."""
import numpy as np
import pytest

from rustybam_amd import trim_driver
from trim_util import CONFIGS, OracleEngine, format_recs, oracle_args, panic_group, parse, random_trim_paf, stats, trim_file


@pytest.mark.parametrize("seed", [1, 2])
def test_generated_files_hold_the_hard_cases(oracle, seed):
    text = trim_file(seed)
    for cfg in CONFIGS:
        rc, out = oracle.cli(*oracle_args(cfg), stdin=text)
        assert rc == 0 and out, cfg
    s = stats(text, oracle)
    assert s["groups"] == 150 and s["records"] > 500, s
    assert s["irregular"] >= 100 and s["irregular_cut"] >= 80, s           # irregular records that trim-paf really cuts
    assert s["irregular_cut_twice"] >= 20, s                                # ... in two passes or more (moved, then cut again)
    assert s["max_group"] >= 40 and s["max_deferred_first_pass"] >= 2, s   # a deep group: deferred pairs, many passes
    assert s["contained"] >= 50 and s["tied_groups"] >= 8, s
    assert s["q_st_zero"] >= 40 and s["q_st_zero_lead_no_query"] >= 3, s
    assert s["to_lines"] >= 60, s
    names = {ln.split(b"\t")[0] for ln in text.splitlines()}
    assert {b"q9", b"q10"} <= names or {b"q1", b"q10"} <= names or {b"q2", b"q19"} <= names, sorted(names)[:20]
    assert any(n.startswith(b"Q") for n in names) and any(b"_alt" in n for n in names)


def test_group_sizes_and_interleaving():
    text = trim_file(1)
    lines = text.splitlines()
    names = [ln.split(b"\t")[0] for ln in lines]
    sizes = sorted(np.unique(names, return_counts=True)[1].tolist())
    assert sizes[0] == 1 and 2 in sizes and 3 in sizes and sizes.count(12) >= 3 and sizes[-1] >= 40
    # the groups are interleaved in the file: the reference's stable sort by name has work to do
    assert sum(a != b for a, b in zip(names, names[1:])) > len(set(names)) * 2


def test_generator_is_deterministic(oracle):
    assert random_trim_paf(7, 12) == random_trim_paf(7, 12)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_host_driver_on_the_oracle_kernels_prints_the_oracle_cli_bytes(oracle, cfg):
    """trim_driver.overlapping_paf_recs with the oracle's normalisation and pair step in place of the engine's: the driver's pass
    bookkeeping and tests/trim_util.py's formatting reproduce the oracle CLI byte for byte on the generated files"""
    c = CONFIGS[cfg]
    text = trim_file(1)
    out = trim_driver.overlapping_paf_recs(OracleEngine(oracle), parse(text), c["scores"], c["remove"], c["policy"])
    rc, want = oracle.cli(*oracle_args(cfg), stdin=text)
    assert rc == 0 and format_recs(out).encode() == want


def test_panic_group_panics_in_the_pair_step(oracle):
    for cfg in CONFIGS:
        assert oracle.cli(*oracle_args(cfg), stdin=trim_file(1) + panic_group())[0] == 101, cfg
    with pytest.raises(RuntimeError, match="trim pair .*status 16"):
        trim_driver.overlapping_paf_recs(OracleEngine(oracle), parse(panic_group()))
