"""The inputs of tests/test_gpu_trim_legacy.py tell the two binary-search policies apart: on the CPU, the per-base oracle cuts every pair
under both and the rows of enough pairs differ.  (Inputs on which the policies agree would let a kernel that ignores the policy pass.)"""
import pytest

from trim_legacy_util import INPUTS, LEGACY, MODERN, SCORES, legacy_batch, oracle_rows, rows_differ


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("ops_range,n_pairs,max_overlap,floor", INPUTS)
def test_the_policies_differ_on_the_legacy_inputs(oracle, ops_range, n_pairs, max_overlap, floor, scores):
    b, left, right = legacy_batch(ops_range, n_pairs, max_overlap, scores)
    mod, _ = oracle_rows(oracle, b, left, right, scores, MODERN)
    leg, _ = oracle_rows(oracle, b, left, right, scores, LEGACY)
    n = int(rows_differ(mod, leg).sum())
    print(f"ops {ops_range}, scores {scores}: {len(left)} pairs, {n} differ between the policies")
    assert len(left) >= n_pairs * 9 // 10  # (the builder drops a pair whose records have fewer than 2 query bases)
    assert n >= floor, f"only {n} of {len(left)} pairs differ between the policies"
