"""The exponential geometry matrix's generator (expo_geometry_util) against the
oracle, on the CPU: every row's input reaches the regime the row exists for.
These are conditions on the input, not measurements of the engine; the kernels
run in tests/test_gpu_expo_geometry.py."""
import numpy as np
import pytest

import pyoracle
from expo_geometry_util import (CACHED_ENTRIES, ENTRIES, FIELD, K_XT_CAP, K_XT_RUN, ROWS, SLAB, THICK_PER_WG,
                                expected_counting, plan_of, rng_of, slab_entries, thick_size)
from geometry_util import THIN

CUS = 256  # the thick batch of a one-workgroup-per-CU engine on a 256-CU device


def _series(batch, key, max_size, unit_s):
    m = batch.key_hash == key
    return pyoracle.expo_series(batch.start_ns[m], batch.end_ns[m], max_size, unit_s)


def _durations(batch, key):
    m = batch.key_hash == key
    return np.where(batch.end_ns[m] > batch.start_ns[m], batch.end_ns[m] - batch.start_ns[m], 0).astype(np.uint64)


def _concat(batches):
    from geometry_util import concat
    return concat(batches)


def test_entries_table_is_the_formula():
    for (cap, M, per_cu), ne in ENTRIES.items():
        assert slab_entries(cap, M, per_cu) == ne, (cap, M, per_cu)
    for M, ne in CACHED_ENTRIES.items():
        e = 256
        while e > 4 and e * M * 2 > 65536:
            e //= 2
        assert e == ne, M
    for row, r in ROWS.items():
        for per_cu in (1,) if r["cap"] == 2048 else (1, 2):
            g = expected_counting(row, per_cu)
            if r["count"] == SLAB:
                assert g["expo_entries"] > 0 and g["expo_bins"] * g["expo_bin_slots"] == r["cap"]
                assert g["expo_bin_slots"] == (16 if r["max_size"] <= 2048 else 8)
                if r["max_size"] <= 5:
                    assert g["expo_entries"] == r["cap"]
    assert sorted(r["max_size"] for r in ROWS.values() if r["cfg"]["key_capacity"] == 1500 and not
                  r["cfg"].get("options")) == [2, 3, 5, 159, 161, 1024, 2048, 2049, 4095, 4096]
    assert sum(r["cfg"].get("unit") == "s" for r in ROWS.values()) == 1


@pytest.mark.parametrize("row", list(ROWS))
def test_generator_reaches_the_rows_regime(row):
    r, p = ROWS[row], plan_of(row)
    M, unit_s, div = r["max_size"], p.cfg.unit == "s", p.div
    thin = p.thin(rng_of(row, "thin"))
    n_thick = thick_size(row, CUS, CUS)
    thick = p.thick(rng_of(row, "thick"), n_thick)
    both = _concat([thin, thick])
    assert len(thin) == THIN and len(thick) == CUS * THICK_PER_WG + 17
    for b in (thin, thick):
        z = float((b.key_hash == 0).mean())
        assert 0.005 < z < 0.015, z
        d = np.where(b.end_ns > b.start_ns, b.end_ns - b.start_ns, 0)
        assert int(d.max()) < 1 << 63

    # every series' ns sum stays an exact u64 within a flush interval
    keys, inv = np.unique(both.key_hash, return_inverse=True)
    d = np.where(both.end_ns > both.start_ns, both.end_ns - both.start_ns, 0).astype(np.float64)
    assert np.bincount(inv, weights=d).max() < 0.9 * 2.0 ** 64
    assert len(keys) - 1 <= r["cfg"]["key_capacity"]

    # wide: the lowest scale of the row, and the top half of the bucket array when it has one past 2,048
    wide_scale = []
    for k in p.wide:
        o = _series(both, k, M, unit_s)
        wide_scale.append(o["scale"])
        if M > 2048:
            dur = _durations(thick, k)
            pos = {pyoracle.expo_index(float(x) / div, o["scale"]) % M for x in dur[dur > 0]}
            assert max(pos) >= 2048, (k, max(pos))

    # narrow-far: settled at scale >= 9 with every index outside the field (the index is monotone in the
    # duration: the band's ends decide), in the thin batch alone as in both
    for b in (thin, both):
        for k in p.narrow:
            o = _series(b, k, M, unit_s)
            assert o["scale"] >= 9, (k, o["scale"])
            assert o["scale"] > max(wide_scale)
            dur = _durations(b, k)
            ends = [pyoracle.expo_index(float(x) / div, o["scale"]) for x in (dur.min(), dur.max())]
            assert dur.min() > 0 and (ends[1] < -FIELD - 1 or ends[0] > FIELD), (k, ends)

    # field-edge: each series settled at its scale in the thin batch already, holding its targets; all six together
    seen = set()
    for j, k in enumerate(p.edge):
        for b in (thin, thick, both):
            o = _series(b, k, M, unit_s)
            assert o["scale"] == p.edge_scale[j], (k, o["scale"], p.edge_scale[j])
            have = {pyoracle.expo_index(float(x) / div, o["scale"]) for x in np.unique(_durations(b, k))}
            assert set(p.edge_targets[j]) <= have, (k, have)
            assert any(-FIELD - 1 <= i <= FIELD for i in have)  # (in-field values pin the scale)
        seen |= set(p.edge_targets[j])
    assert seen == {-FIELD - 2, -FIELD - 1, -FIELD, FIELD - 1, FIELD, FIELD + 1}

    # single
    for b in (thin, thick):
        for j, k in enumerate(p.single):
            o = _series(b, k, M, unit_s)
            assert o["count"] > 0
            if j < 2:
                assert (o["scale"], len(o["counts"]), o["zero_count"]) == (20, 1, 0)
            elif j < 4 or j >= 6:
                assert o["zero_count"] == o["count"] and len(o["counts"]) == 0
            else:
                assert 0 < o["zero_count"] < o["count"] and len(o["counts"]) == 1
        m = np.isin(b.key_hash, p.single[6:])
        assert (b.end_ns[m] < b.start_ns[m]).all()

    # hot / cold: half the spans on 8 series; the positive-duration series outnumber the entries wherever the
    # entries do not cover the table's keys anyway
    for b, hot in ((thin, p.thin_hot), (thick, p.thick_hot)):
        share = float(np.isin(b.key_hash, hot).mean())
        assert 0.47 < share < 0.53, share
    posd = thick.end_ns > thick.start_ns
    cold = np.setdiff1d(np.unique(thick.key_hash[posd & (thick.key_hash != 0)]), p.thick_hot)
    if r["cfg"]["key_capacity"] == 1500:
        assert len(cold) >= 1400
    for per_cu in (1,) if r["cap"] == 2048 else (1, 2):
        ne = expected_counting(row, per_cu)["expo_entries"]
        if r["count"] == SLAB and ne < r["cfg"]["key_capacity"]:
            assert len(cold) > ne, (len(cold), ne)

    # the thick launch: half its hot and heavy series and the odd cold ones are not in the thin batch, the settled
    # ones have six spans there; neither holds an entry, so a workgroup's share of tail records passes the record
    # buffer; each heavy series alone passes a run
    absent = ~np.isin(thick.key_hash, np.unique(thin.key_hash)) & posd & (thick.key_hash != 0)
    settled = p.bulk[p.settled]
    light = np.isin(thick.key_hash, settled) & posd
    assert absent.mean() * THICK_PER_WG > K_XT_CAP // 2 and light.mean() * THICK_PER_WG > K_XT_CAP // 4
    tk, tn = np.unique(thin.key_hash[(thin.end_ns > thin.start_ns) & (thin.key_hash != 0)], return_counts=True)
    assert (tn[np.isin(tk, settled)] == 6).all() and np.isin(settled, tk).all()
    for k in settled:  # the thin batch settles the scale: the thick batch's values lie inside its range
        assert _series(thin, k, M, unit_s)["scale"] == _series(both, k, M, unit_s)["scale"]
    for per_cu in (1,) if r["cap"] == 2048 else (1, 2):
        ne = expected_counting(row, per_cu)["expo_entries"]
        if r["count"] == SLAB and ne <= 397:  # the settled series hold no entry: at least ne series have 8 spans
            assert int((tn >= 8).sum()) >= ne, (int((tn >= 8).sum()), ne)
            assert (absent | light).mean() * THICK_PER_WG > K_XT_CAP
    for k in p.heavy:
        assert (thick.key_hash == k).mean() * THICK_PER_WG > 4 * K_XT_RUN
    assert np.isin(thick.key_hash, p.heavy).sum() >= 0.25 * (~np.isin(thick.key_hash, p.thick_hot)).sum()


@pytest.mark.parametrize("row", list(ROWS))
def test_moving_scales_drop(row):
    """Launch B's far value takes half of the narrow-far series down by at
    least 8 scales; the others stay; launch C is narrow again."""
    r, p = ROWS[row], plan_of(row)
    M, unit_s = r["max_size"], p.cfg.unit == "s"
    a, b, c = p.moving(rng_of(row, "moving"))
    assert set(np.unique(a.key_hash)) - {0} == set(int(k) for k in p.narrow)
    moved = 0
    for j, k in enumerate(p.narrow):
        sa, sb = _series(a, k, M, unit_s)["scale"], _series(_concat([a, b]), k, M, unit_s)["scale"]
        sc = _series(c, k, M, unit_s)["scale"]
        assert sa >= 9 and sc == sa, (k, sa, sc)
        if p.narrow_far[j]:
            moved += 1
            da, far = _durations(a, k), float(p.narrow_far[j])
            assert abs(np.log2(far / float(da.max()))) >= 40 and abs(np.log2(far / float(da.min()))) >= 40
            assert sa - sb >= 8, (k, sa, sb)
        else:
            assert sb == sa
    assert moved * 2 == len(p.narrow)
