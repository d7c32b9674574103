"""Inputs of the legacy-policy trim-paf tests (tests/test_trim_legacy_inputs.py on the CPU, tests/test_gpu_trim_legacy.py on the device):
pairs of regular records whose cut depends on which duplicate of qpos_aln the binary search returns -- a D behind the last base of a
query op inside the overlap -- and the comparison that says whether two sets of pair rows differ."""
import zlib

import numpy as np

import rustybam_amd
from rbtest_util import random_cigar, sums
from test_gpu_trim import _pairs_batch

MODERN, LEGACY = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY
# (ops range, pairs, max overlap, floor on the pairs whose rows differ between the policies)
INPUTS = [((3, 60), 300, None, 20), ((60, 200), 100, None, 20), ((2000, 9000), 24, 4000, 3)]
SCORES = [(1, 1, 1), (2, 3, 5)]
ROW_FIELDS = ("t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_n")


def legacy_batch(ops_range, n_pairs, max_overlap, scores):
    rng = np.random.default_rng(zlib.crc32(f"legacy{ops_range}{scores}".encode()))
    return _pairs_batch(rng, n_pairs, "regular", ops_range=ops_range, max_overlap=max_overlap)


def oracle_rows(oracle, b, left, right, scores, policy):
    ob = oracle.Batch(b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"], np.zeros(len(b["t_st"]), np.uint32))
    return oracle.overlap_split(ob, left, right, scores, policy)


def rows_differ(a, b):
    """per pair: status, split index, split score, either side's coordinates, nmatch, aln_len or out_n differ"""
    d = (a["status"] != b["status"]) | (a["split_idx"] != b["split_idx"]) | (a["split_score"] != b["split_score"])
    for k in ROW_FIELDS:
        d |= (a[k] != b[k]).any(axis=1)
    return d


def odd_geometries(seed=99):
    """regular records whose query spans do not overlap, touch, coincide, or contain one another (the shapes of
    test_gpu_trim.py::test_pairs_odd_geometries): the split degenerates and the clips run into the reference's panics"""
    rng = np.random.default_rng(seed)
    cig, t_st, t_en, q_st, q_en, strand, left, right = [], [], [], [], [], [], [], []
    for rel in ("apart", "touch", "same", "contained", "contains", "one_base", "apart", "same", "contained"):
        for sa in "+-":
            for sb in "+-":
                ca = random_cigar(rng, int(rng.integers(5, 90)), "regular")
                cb = random_cigar(rng, int(rng.integers(5, 90)), "regular")
                (ra, qa), (rb, qb) = sums(ca), sums(cb)
                a0 = int(rng.integers(0, 3)) * 500
                if rel == "apart":
                    b0 = a0 + qa + 17
                elif rel == "touch":
                    b0 = a0 + qa
                elif rel == "one_base":
                    b0 = a0 + qa - 1
                elif rel == "same":
                    cb, rb, qb, b0 = ca, ra, qa, a0
                elif rel == "contained":
                    if qb >= qa:
                        ca, cb, ra, rb, qa, qb = cb, ca, rb, ra, qb, qa
                    b0 = a0 + (qa - qb) // 2
                else:
                    b0 = a0 + max(qa // 3, 1)
                for c, r, q, s0, sd in ((ca, ra, qa, a0, sa), (cb, rb, qb, b0, sb)):
                    ts = int(rng.integers(0, 5000))
                    cig.append(c); t_st.append(ts); t_en.append(ts + r); q_st.append(s0); q_en.append(s0 + q); strand.append(ord(sd))
                left.append(len(cig) - 2); right.append(len(cig) - 1)
    off = np.zeros(len(cig) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in cig])
    b = dict(ops=np.concatenate(cig), op_off=off, t_st=np.array(t_st, np.uint64), t_en=np.array(t_en, np.uint64),
             q_st=np.array(q_st, np.uint64), q_en=np.array(q_en, np.uint64), strand=np.array(strand, np.uint8))
    return b, np.array(left, np.uint32), np.array(right, np.uint32)
