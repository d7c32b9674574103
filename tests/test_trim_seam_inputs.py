"""What the inputs of tests/test_gpu_trim_seams.py hold (tests/trim_seam_util.py), proved on the CPU: every record is regular and passes the
oracle's scan untouched, the oracle cuts every pair (status OK; the status cases: the statuses they name), the overlap's ends lie in the ops
the case planted, and the regions and routes follow from the restatement of the cascade's sizes.  Prints, per pair, n, ia, ib, the regions and
the expected route (pytest -s shows it)."""
import time

import numpy as np
import pytest

import trim_seam_util as u

NAMES = list(u.CASES)
ROW_REASONS = {(T, r) for T in u.ROW_T for r in (3, 4, 7, "multi")}
WAVE_REASONS = {("wave", cap) for cap in u.WAVE_CAPS}


def _oracle_rows(oracle, c, scores, policy):
    args, left, right = c.args()
    return oracle.overlap_split(oracle.Batch(*args), left, right, scores, policy)


def _describe(c, i, legacy):
    g = c.geometry(i)
    if g is None:
        return f"{c.name}[{i}] {c.notes[i]}: spans do not overlap"
    out = []
    for w, xa, xb in g:
        n, ia, ib, q = len(w), u.op_of(w, xa), u.op_of(w, xb), int(u.qpre(w)[-1])
        rows = [u.row_region(n, T, xa, xb, q)[1:] for T in u.ROW_T]
        cap = next((cp for cp in u.WAVE_CAPS if u.wave_fits(n, cp, ia, ib)), None)
        wave = u.wave_region(n, cap, ia, ib) if cap else None
        out.append(f"n={n} ia={ia} ib={ib} row regions {[(a, a + m) for a, m in rows]} wave region {wave} under {cap}")
    route, why = u.predict(g, legacy)
    return f"{c.name}[{i}] {c.notes[i]}: L {out[0]}; R {out[1]}; route {route if c.route_open is None else 'open'} declines {sorted(map(str, why))}"


@pytest.mark.parametrize("name", NAMES)
def test_records_are_regular_and_the_oracle_cuts_every_pair(oracle, name):
    c = u.case(name)
    args, left, right = c.args()
    ob = oracle.Batch(*args)
    norm = oracle.normalize(ob)
    assert len(left) == len(c.notes) > 0
    for r, (w, nr) in enumerate(zip(c.cigs, norm)):
        assert u.is_regular(w), (name, r)
        assert nr["status"] == 0 and nr["first_op"] == 0 and nr["n_ops"] == len(w) and nr["lead_ops"] == 0 and nr["trail_ops"] == 0, (name, r)
        assert int(nr["q_st"]) == int(args[4][r]) and int(nr["q_en"]) == int(args[5][r]) and int(nr["t_en"]) == int(args[3][r]), (name, r)
    for policy in c.policies:
        rows, _ = _oracle_rows(oracle, c, c.scores[0], policy)
        if c.status is not None:
            assert (rows["status"] == c.status).all(), (name, policy, rows["status"])
        for i in range(len(left)):
            print(_describe(c, i, policy == u.LEGACY), "oracle status", int(rows["status"][i]))


PLANTED = [n for n in NAMES if n.startswith(("row_", "wave_", "checkpoints")) and n != "wave_direction"]


@pytest.mark.parametrize("name", PLANTED)
def test_the_split_of_a_planted_pair_lies_inside_the_overlap(oracle, name):
    """the route follows from the sizes only as long as the clip does not ask for the op in front of the overlap's far op (a region that starts
    there declines such a clip: `bad`, decline 5 / 6): the partner is built so that the split is never the overlap's far end"""
    c = u.case(name)
    args, left, right = c.args()
    n_ovl = np.minimum(args[5][left], args[5][right]) - np.maximum(args[4][left], args[4][right])
    planted_left = (np.arange(len(left)) % 4) < 2
    for policy in c.policies:
        for scores in c.scores:
            rows, _ = _oracle_rows(oracle, c, scores, policy)
            assert (rows["split_idx"][planted_left] > 0).all() and (rows["split_idx"][~planted_left] < n_ovl[~planted_left]).all(), (name, policy, scores)


def _plants(c, legacy):
    """(route, reasons) of every plant: the four pairs of a plant agree"""
    r = c.routes(legacy)
    assert len(r) % 4 == 0
    out = []
    for k in range(0, len(r), 4):
        assert all(x == r[k] for x in r[k:k + 4]), (c.name, k, r[k:k + 4])
        out.append(r[k])
    return out


def test_row_cases_lie_on_the_row_form_s_thresholds():
    c = u.case("row_length")
    assert sorted({len(w) for w in c.cigs if len(w) > 40}) == [63, 64, 65, 127, 128, 129] and min(len(w) for w in c.cigs) < 30
    for legacy in (False, True):
        # 63, 64: staged whole by both attempts; 65: a region at either end; 127, 128: whole under T = 8; 129: a from-end region under both
        assert all(x == ("row", set()) for x in _plants(c, legacy))
    sub = [w for w in c.cigs if len(w) == 65]
    q = int(u.qpre(sub[0])[-1])
    assert u.row_region(65, 4, q - 20, q - 1, q) == (True, 1, 64) and u.row_region(65, 4, 0, 19, q) == (False, 0, 64)
    assert u.row_region(64, 4, q - 20, q - 1, q) == (False, 0, 64) and u.row_region(129, 8, q - 20, q - 1, q)[:2] == (True, 1)
    c = u.case("row_edge")
    want = [("row", set()), ("row", set()), ("row", {(4, 4)}), ("row", {(4, 4)}), ("row", {(4, 4)}), ("wave", {(4, 4), (8, 4)}),
            ("row", {(4, 7)}), ("row", {(4, 7)}), ("row", set()), ("row", {(4, 4)}), ("wave", {(4, 4), (8, 7)}), ("wave", {(4, 4), (8, 7)})]
    for legacy in (False, True):
        got = _plants(c, legacy)
        assert [(r, {x for x in why if x[0] != "wave"}) for r, why in got] == want, got
    c = u.case("row_chunks")
    none, m48 = set(), {(4, "multi"), (8, "multi")}
    want = {False: [("row", {(4, 3)}), ("row", none), ("wave", {(4, 3), (8, 3)}), ("row", none), ("row", none), ("row", none)],
            True: [("wave", {(4, 3), (8, "multi")}), ("wave", m48), ("wave", {(4, 3), (8, 3)}), ("wave", m48), ("row", none), ("row", none)]}
    for legacy in (False, True):
        assert _plants(c, legacy) == want[legacy], (legacy, _plants(c, legacy))


def test_wave_cases_lie_on_the_wave_form_s_thresholds():
    for name in ("wave_length", "wave_steps", "checkpoints"):
        for legacy in (False, True):
            assert all(r == "wave" and {(4, 4), (8, 4)} <= why for r, why in _plants(u.case(name), legacy)), name
    for cap, nxt in zip(u.WAVE_CAPS, u.WAVE_CAPS[1:] + (None,)):
        c = u.case(f"wave_fit_{cap}")
        got = _plants(c, False)
        assert got == _plants(c, True)
        for k, (route, why) in enumerate(got):  # tail exact, tail + 1, head exact, head + 1
            over = k & 1
            w = c.cigs[c.left[4 * k]]           # (the first pair of a plant has the planted record on the left)
            g = c.geometry(4 * k)[0]
            i0, i1 = u.wave_region(len(w), cap, u.op_of(w, g[1]), u.op_of(w, g[2]))
            assert i1 - i0 == cap + over and len(w) > cap, (cap, k, i0, i1)
            assert (("wave", cap) in why) == bool(over) and route == ("serial" if over and nxt is None else "wave"), (cap, k, route, why)
    # step geometry: the regions the planted lanes give
    R = lambda n, ia, ib: u.wave_region(n, 192, ia, ib)  # noqa: E731
    assert R(400, 15, 399) == (0, 400) and R(400, 16, 399) == (0, 400) and R(400, 207, 399) == (128, 400) and R(400, 208, 399) == (192, 400)
    assert R(500, 0, 174) == (0, 191) and R(500, 0, 175) == (0, 192) and R(500, 0, 191) == (0, 208) and R(260, 0, 258) == (0, 260)
    assert R(320, 170, 319) == (154, 320) and R(321, 171, 320) == (155, 321) and not u.wave_fits(1100, 1024, 10, 1099)
    # the direction case: xa - (Qtot - 1 - xb) = -2, 0, 2 on '+' (the sign turns on '-'), and the walk into step 0 whose region fits 192 ops
    c = u.case("wave_direction")
    for i, note in enumerate(c.notes):
        w, xa, xb = c.geometry(i)[0]
        d = xa - (int(u.qpre(w)[-1]) - 1 - xb)
        if note.startswith("xa -"):
            assert abs(d) == abs(int(note.split("=")[1])) and 0 < xa and xb < int(u.qpre(w)[-1]) - 1
        else:
            ia, ib = u.op_of(w, xa), u.op_of(w, xb)
            assert d > 0 and len(w) > 192 and ia == 3 and u.wave_region(len(w), 192, ia, ib) == (0, ib + 17) and ib + 17 <= 192
    # checkpoints: chunks of the staged regions, and the last, partial group of the 64-ary descent
    for m, stride, last in ((1025, 2, 1), (4097, 5, 2), (6000, 6, 3), (4096, 4, 4)):
        chunks = (m + 15) // 16
        assert chunks > 64 and (chunks + 63) // 64 == stride and chunks - (chunks - 1) // stride * stride == last
    assert u.wave_region(6400, 6144, 2320, 6399) == (2304, 6400)


def test_ties_hold_the_named_property_in_the_oracle_s_result(oracle):
    c = u.case("ties")
    for policy in c.policies:
        rows, _ = _oracle_rows(oracle, c, (1, 1, 1), policy)
        for l_ov, r_ov, prop, at in c.strings:
            f = u.f_values(l_ov, r_ov, (1, 1, 1))
            idx, best = u.first_strict_max(f)
            print(f"ties: {prop}: n={len(l_ov)} f(0)={f[0]} max={f.max()} at {np.flatnonzero(f == f.max())[:4]} -> split {idx}, score {best}")
            assert (rows["split_idx"][at:at + 4] == idx).all() and (rows["split_score"][at:at + 4] == best).all(), (prop, rows["split_idx"][at:at + 4])
            top = np.flatnonzero(f == f.max())
            if prop.startswith("all f"):
                assert f.max() <= 0 and f[0] < 0 and (idx, best) == (0, 0)
            elif prop.startswith("flat"):
                assert (f == f[0]).all() and idx == 0 and best == max(int(f[0]), 0)
            elif prop.startswith("maximum only"):
                assert top.tolist() == [len(l_ov)] == [idx]
            elif "twice" in prop:
                assert len(top) == 2 and idx == top[0] and f[0] < f.max() and top[1] < len(l_ov)
            elif prop.startswith("a plateau"):
                assert len(top) > 10 and idx == top[0] > 0 and top[-1] == len(l_ov)
            else:
                assert top.tolist() == [12] == [idx]
    # where the tied candidates lie: ops apart in the left record ('+': op order = query order)
    for l_ov, r_ov, prop, at in c.strings:
        if "twice" in prop:
            w = c.cigs[c.left[at]]
            f = u.f_values(l_ov, r_ov, (1, 1, 1))
            k1, k2 = np.flatnonzero(f == f.max())
            xa = c.geometry(at)[0][1]
            apart = u.op_of(w, xa + k2) - u.op_of(w, xa + k1)
            assert apart == {"(small)": 13, "64 ops apart (large)": 64, "70 ops apart (large)": 71}[prop.split("twice")[1].strip(", ")], (prop, apart)
            assert (20 <= len(w) <= 60) == ("small" in prop)
            if "large" in prop:
                assert all(r == "wave" for r, _ in c.routes(False)[at:at + 4])
    # the special last base: with the left record on '+' the maximum lies in front of the base the D run behind its op rescores
    c = u.case("special_max")
    for scores in c.scores:
        rows, _ = _oracle_rows(oracle, c, scores, u.MODERN)
        assert (rows["split_idx"][:2] == 8).all(), rows["split_idx"][:8]
        w = c.cigs[c.left[0]]
        ia = u.op_of(w, c.geometry(0)[0][1])
        assert (int(w[ia]) >> 4) - (c.geometry(0)[0][1] - int(u.qpre(w)[ia])) == 9 and int(w[ia + 1]) & 15 == u.D  # nine bases of the op, then the D


def test_one_op_cases_keep_one_op(oracle):
    c = u.case("one_op")
    rows, _ = _oracle_rows(oracle, c, (1, 1, 1), u.MODERN)
    want = {"split at 0": 0, "split at n:": 12, "split at n - 1": 11, "split at 1": 1}
    for i, note in enumerate(c.notes):
        for k, v in want.items():
            if note.startswith(k):
                assert int(rows["split_idx"][i]) == v, (note, rows["split_idx"][i])
    one = [i for i in range(len(rows)) if 1 in rows["out_n"][i].tolist()]
    assert len(one) >= 16
    assert sum(len(w) == 1 for w in c.cigs) == 16


def test_every_route_and_decline_is_expected_somewhere():
    routes, reasons = set(), set()
    for name in NAMES:
        c = u.case(name)
        if c.route_open is not None:
            continue
        for legacy in (False, True):
            for r, why in c.routes(legacy):
                routes.add(r)
                reasons |= why
    assert routes == {"row", "wave", "serial"}
    assert ROW_REASONS <= reasons and WAVE_REASONS <= reasons, (ROW_REASONS | WAVE_REASONS) - reasons
    open_cases = {n: u.case(n).route_open for n in NAMES if u.case(n).route_open}
    assert set(open_cases) == {"wave_direction", "statuses"}
    c = u.case("statuses")
    assert {n.split()[0] for n in c.notes} == set(u.STATUS_OF) and {len(w) for w in c.cigs} == {61, 193, 1025}


def test_status_cases_name_what_the_oracle_says(oracle):
    c = u.case("statuses")
    for policy in c.policies:
        rows, _ = _oracle_rows(oracle, c, (1, 1, 1), policy)
        for note, st in zip(c.notes, rows["status"]):
            assert int(st) == u.STATUS_OF[note.split()[0]], (note, int(st))


def test_walker_batch_fills_a_second_round_and_the_oracle_is_quick(oracle):
    t0 = time.time()
    args, left, right, is_slab, short, slab = u.walker_batch()
    t1 = time.time()
    assert (~is_slab).sum() == 12288 and is_slab.sum() == 64 and len(left) > u.SLABS * u.WALK * 4
    for legacy in (False, True):
        assert all(r == "row" and why == {(4, 4)} for r, why in short.routes(legacy))
        assert all(r == "wave" and why >= {(4, 4), (8, 4), ("wave", 6144)} for r, why in slab.routes(legacy))
    for c, lo, hi, n in ((short, 70, 100, 140), (slab, 6200, 7000, 7100)):
        for i in range(len(c.left)):
            w, xa, xb = next(g for g in c.geometry(i) if len(g[0]) == n)
            assert lo <= u.op_of(w, xb) - u.op_of(w, xa) + 1 <= hi
    pos = np.flatnonzero(is_slab)
    assert np.diff(pos).min() > 150 and pos[0] > 50       # spread through the batch
    rows, _ = oracle.overlap_split(oracle.Batch(*args), left, right, (1, 1, 1), u.MODERN)
    t2 = time.time()
    assert (rows["status"] == 0).all()
    print(f"walker batch: {len(left)} pairs, {int(args[1][-1])} ops, built in {t1 - t0:.2f} s, oracle {t2 - t1:.2f} s")
    assert t2 - t1 < 10
