"""What tests/hll_util.py's crafted trace ids are, proven without a GPU.

For every row tests/test_gpu_hll_ids.py runs (geometry_util.RING_ROWS and
hll_util.HLL_ROWS) and every family: the claimed (index, rho) of each span is
what the plain-Python forward hash gives its trace id; the oracle fed the
batch holds exactly the claimed maxima and nothing else; every rho 1 .. 65 - p
is claimed; position 0 and the last register are claimed; no crafted span is
invalid.  The NumPy forms of the hash, forwards and backwards, equal the
scalar ones on random and edge values, and the forward hash equals the
oracle's xxh64.
"""
import numpy as np
import pytest

import hll_util as hu
import pyoracle
from geometry_util import expected_oor, key_pool, ring_start
from hll_util import ALL_ROWS, FLOOR, Ring, config_of

EDGES = (0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1)
ROW_NAMES = list(ALL_ROWS)


def _oracle(cfg, batches):
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for b in batches:
        o.ingest(b)
    return o


def _registers(o, ring):
    seen = set(o.window_ids())
    zero = np.zeros((ring.S, ring.m), np.uint8)
    return {w: o.window(w)[0] if w in seen else zero for w in range(ring.w0, ring.w0 + ring.W)}


def _assert_scalar(batch, claims, p, pick=None):
    """The claims against the plain-Python reference, span by span."""
    for i in (range(len(batch)) if pick is None else pick):
        x = hu.xxh64_16(int(batch.trace_w0[i]), int(batch.trace_w1[i]))
        assert hu.index_rho(x, p) == (int(claims[i, 2]), int(claims[i, 3])), i


def _assert_valid(batch, claims, cfg, ring, n_keys):
    assert np.array_equal(claims[:, 0], (batch.end_ns // np.uint64(cfg.window_ns)).astype(np.int64))
    assert np.array_equal(claims[:, 1], (batch.meta & np.uint32(0xFFFF)).astype(np.int64))
    assert ((claims[:, 0] >= ring.w0) & (claims[:, 0] < ring.w0 + ring.W)).all()
    assert ((claims[:, 1] >= 0) & (claims[:, 1] < ring.S)).all()
    assert (batch.key_hash != 0).all() and np.isin(batch.key_hash, key_pool(n_keys)).all()
    assert (batch.start_ns < batch.end_ns).all()
    assert expected_oor([batch], cfg, ring.w0) == 0


def _assert_oracle(batches, claims, cfg, ring):
    o = _oracle(cfg, batches)
    got, want = _registers(o, ring), hu.expected_registers(ring, claims)
    for w in want:
        assert np.array_equal(got[w], want[w]), w
    st = o.stats()
    assert st["invalid_service"] == 0 and st["zero_key"] == 0 and st["spans"] == sum(len(b) for b in batches)
    assert set(o.window_ids()) <= set(want)
    return got


def test_forward_reference_vs_oracle_xxh64():
    rng = np.random.default_rng(1)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [tuple(int(v) for v in rng.integers(0, 2**64, 2, dtype=np.uint64))
                                                     for _ in range(1000)]
    for w0, w1 in pairs:
        assert hu.xxh64_16(w0, w1) == pyoracle.xxh64(w0.to_bytes(8, "little") + w1.to_bytes(8, "little")), (w0, w1)


def test_array_forms_equal_the_scalar_ones():
    rng = np.random.default_rng(2)
    edges = np.array(EDGES, np.uint64)
    a = np.concatenate([rng.integers(0, 2**64, 10_000, dtype=np.uint64), np.repeat(edges, len(edges))])
    b = np.concatenate([rng.integers(0, 2**64, 10_000, dtype=np.uint64), np.tile(edges, len(edges))])
    w1 = hu.trace_with_hash_np(a, b)
    fwd = hu.xxh64_16_np(a, b)
    assert w1.dtype == np.uint64 and fwd.dtype == np.uint64
    for i in range(len(a)):
        x, w0 = int(a[i]), int(b[i])
        assert int(w1[i]) == hu.trace_with_hash(x, w0), (x, w0)
        assert int(fwd[i]) == hu.xxh64_16(x, w0), (x, w0)
    # backwards then forwards is the identity
    assert np.array_equal(hu.xxh64_16_np(b, w1), a)
    for p in (4, 10, 11, 14, 18):
        index, rho = hu.index_rho_np(a, p)
        for i in range(0, len(a), 7):
            assert (int(index[i]), int(rho[i])) == hu.index_rho(int(a[i]), p)
        edge = [hu.index_rho(x, p) for x in EDGES]
        assert edge[0] == (0, 65 - p) and edge[1] == (0, 64 - p) and edge[5] == ((1 << p) - 1, 1)


def test_hashes_builder():
    for p in (4, 14, 18):
        top = 65 - p
        for low in (0, hu._M64, hu.ALT):
            x = hu.hashes(p, np.full(top, 5), np.arange(1, top + 1), np.full(top, low, np.uint64))
            assert [hu.index_rho(int(v), p) for v in x] == [(5, r) for r in range(1, top + 1)]
        assert int(hu.hashes(p, [3], [top], [hu._M64])[0]) == 3 << (64 - p)  # the sentinel alone ends the count


@pytest.mark.parametrize("row", ROW_NAMES)
def test_crafted_families(row):
    cfg, n_keys = config_of(row), ALL_ROWS[row]["n_keys"]
    w0 = ring_start(cfg)
    ring, p = Ring(cfg, w0), cfg.hll_p
    top = ring.top
    for touch_zero in (True, False):
        used = set()
        blocks, bl_c = hu.shared_word(cfg, w0, n_keys, used)
        er, er_c = hu.every_rho(cfg, w0, n_keys, touch_zero, used)
        hb, hb_c = hu.half_boundary(cfg, w0, n_keys, used)
        for b, c in [(er, er_c), (hb, hb_c)] + list(zip(blocks, bl_c)):
            assert len(b) == len(c)
            _assert_scalar(b, c, p)
            _assert_valid(b, c, cfg, ring, n_keys)
            _assert_oracle([b], c, cfg, ring)

        # every_rho: each (rho, variant) on a register of its own, every rho there in its three variants
        pos = ring.pos(er_c[:, 0], er_c[:, 1], er_c[:, 2])
        assert len(set(pos)) == len(pos) >= 3 * top
        assert sorted(set(er_c[:, 3])) == list(range(1, top + 1))
        x = hu.xxh64_16_np(er.trace_w0, er.trace_w1)
        tail = x & np.uint64((1 << (64 - p)) - 1)
        for r in range(1, top + 1):
            t = [int(v) for v in tail[:3 * top][er_c[:3 * top, 3] == r]]
            lead = 1 << (64 - p - r) if r < top else 0
            below = lead - 1 if lead else 0
            assert len(t) == 3 and set(t) == {lead | (m & below) for m in (0, hu._M64, hu.ALT)}, (r, t)
            assert len(set(t)) == (3 if r < top - 2 else 2 if r == top - 2 else 1)
        claimed = {int(q): int(r) for q, r in zip(pos, er_c[:, 3])}
        assert (ring.zero in claimed) == touch_zero and claimed.get(ring.zero, top) == top
        assert claimed[ring.last] == top - 1 and ring.regs - 1 in claimed
        assert tuple(int(v) for v in ring.unpos(ring.last)) == (w0 + ring.W - 1, ring.S - 1, ring.m - 1)

        # half_boundary: around bit 32 of x << p
        assert sorted(set(hb_c[:, 3])) == [31, 32, 33, 34] and len(hb) == 20
        hpos = ring.pos(hb_c[:, 0], hb_c[:, 1], hb_c[:, 2])
        assert len(set(hpos) | set(pos)) == len(hpos) + len(pos)
        xs = [hu.xxh64_16(int(a), int(b)) for a, b in zip(hb.trace_w0, hb.trace_w1)]
        pm = (1 << p) - 1
        for r in (31, 32, 33, 34):
            ys = [(v << p) & hu._M64 for v, c in zip(xs, hb_c) if c[3] == r]
            yh, yl = {y >> 32 for y in ys}, {y & 0xFFFFFFFF for y in ys}
            assert yh == {31: {2, 3}, 32: {1}, 33: {0}, 34: {0}}[r], (r, yh)
            assert len(yl) >= 3  # the low half varies under one rho (p = 18: the low p bits are all there is)
            below = (1 << (64 - p - r)) - 1
            lows = {v & pm & below for v, c in zip(xs, hb_c) if c[3] == r}
            assert {0, pm & below} <= lows and pm & below

        # shared_word: one aligned word, one (register, rho) a wave step, a ceiling and below
        wpos = ring.pos(bl_c[0][:, 0], bl_c[0][:, 1], bl_c[0][:, 2])
        assert len(blocks[0]) == 256 and wpos[0] % 4 == 0 and np.array_equal(wpos, np.tile(wpos[0] + np.arange(4), 64))
        ladders = bl_c[0][:, 3].reshape(64, 4)
        assert (np.diff(ladders[:, 0]) >= 0).all() and (np.diff(ladders[:, 1]) <= 0).all()
        assert (ladders[0, 0], ladders[-1, 0]) == (1, top)
        for k in (2, 3):
            assert sorted(ladders[:, k]) == list(ladders[:, 0]) and (np.diff(ladders[:, k]) < 0).any()
        assert len(blocks[1]) == 128 and len(set(map(tuple, bl_c[1]))) == 1
        assert len(set(blocks[1].trace_w1)) == 128
        assert bl_c[2][0, 3] == top and set(bl_c[2][1:, 3]) == set(range(1, top))
        assert len(set(map(tuple, bl_c[2][:, :3]))) == 1
        others = np.concatenate([ring.pos(c[:, 0], c[:, 1], c[:, 2]) for c in bl_c])
        assert not set(others) & (set(pos) | set(hpos))

        # together: every rho visible as a register's final value
        singles, blocks2, claims = hu.crafted(cfg, w0, n_keys, touch_zero)
        got = _assert_oracle([singles] + blocks2, claims, cfg, ring)
        values = set(np.concatenate([v.ravel() for v in got.values()]))
        assert set(range(1, top + 1)) <= values
        assert (got[int(ring.unpos(0)[0])][0, 0] == top) == touch_zero

        # shuffled into random traffic
        batch, alone, claims2 = hu.mixed(cfg, w0, n_keys, touch_zero)
        assert np.array_equal(claims2, claims) and np.array_equal(hu.claims_of(alone, cfg), claims)
        ids = set(zip(alone.trace_w0.tolist(), alone.trace_w1.tolist()))
        assert (int(batch.trace_w0[0]), int(batch.trace_w1[0])) in ids
        assert (int(batch.trace_w0[-1]), int(batch.trace_w1[-1])) in ids
        assert len(batch) % 4 != 0 and len(batch) > 2 * 2048  # more than one workgroup, a ragged end
        at = int(np.flatnonzero(batch.trace_w1 == blocks2[0].trace_w1[0])[0])
        assert at % 128 == 0 and np.array_equal(batch.trace_w1[at:at + 256], blocks2[0].trace_w1)
        at = int(np.flatnonzero(batch.trace_w1 == blocks2[1].trace_w1[0])[0])
        assert at % 128 == 0 and np.array_equal(batch.trace_w1[at:at + 128], blocks2[1].trace_w1)
        c = hu.claims_of(batch, cfg)
        inside = (c[:, 1] < ring.S) & (c[:, 0] >= w0) & (c[:, 0] < w0 + ring.W)
        on_zero = int((ring.pos(c[inside, 0], c[inside, 1], c[inside, 2]) == 0).sum())
        assert on_zero >= 1 if touch_zero else on_zero == 0
        regs = _registers(_oracle(cfg, [batch]), ring)
        want = hu.expected_registers(ring, claims)
        for w in want:  # random traffic only adds: no crafted value is lost, the high ones stand
            assert (regs[w] >= want[w]).all() and np.array_equal(regs[w][want[w] > 30], want[w][want[w] > 30])


@pytest.mark.parametrize("row", ["ring_default", "ring_1024_noerr", "ring_binned", "ring_part"])
def test_invalid_spans(row):
    cfg, n_keys = config_of(row), ALL_ROWS[row]["n_keys"]
    w0 = ring_start(cfg)
    ring = Ring(cfg, w0)
    b = hu.invalid_spans(cfg, w0, n_keys)
    c = hu.claims_of(b, cfg)
    _assert_scalar(b, c, cfg.hll_p)
    assert set(c[:, 3]) == {ring.top, ring.top - 1} and set(c[:, 2]) == {0}
    o = _oracle(cfg, [b])
    assert not [w for w in o.window_ids() if w0 <= w < w0 + ring.W and o.window(w)[0].any()]
    n_bad = int((c[:, 1] >= ring.S).sum())
    assert o.stats()["invalid_service"] == n_bad == (len(b) + 1) // 2
    assert expected_oor([b], cfg, w0) == len(b) - n_bad
    assert {int(w) for w in c[c[:, 1] < ring.S, 0]} == {w0 - 1, w0 + ring.W}


@pytest.mark.parametrize("row", ROW_NAMES + [hu.DEEP])
def test_filter_floor_batches(row):
    cfg, n_keys = config_of(row), hu.row_of(row)["n_keys"]
    deep = row == hu.DEEP
    w0 = ring_start(cfg)
    ring, p = Ring(cfg, w0), cfg.hll_p
    shift, n_sb = hu.filter_geometry(row)
    size = 1 << shift
    ff = hu.filter_floor(cfg, w0, n_keys, (shift, n_sb), partial=deep)
    F = FLOOR
    assert len(ff.floor) == len(ff.floored) << shift <= 2**19
    assert len(ff.floored) == (9 if deep else n_sb) and (shift == 13 if deep else shift <= 10)

    # floor: one span per register; F but in the low registers; the claims by the scalar reference on the
    # low registers and a sample, by the array form (test_array_forms_equal_the_scalar_ones) on all
    fpos = ring.pos(ff.floor_claims[:, 0], ff.floor_claims[:, 1], ff.floor_claims[:, 2])
    assert np.array_equal(np.sort(fpos).reshape(-1, size), (ff.floored[:, None] << shift) + np.arange(size)[None, :])
    is_low = np.isin(fpos, ff.low)
    assert (ff.floor_claims[is_low, 3] == 1).all() and (ff.floor_claims[~is_low, 3] == F).all()
    assert np.array_equal(hu.claims_of(ff.floor, cfg), ff.floor_claims)
    _assert_scalar(ff.floor, ff.floor_claims, p, pick=list(np.flatnonzero(is_low)) + list(range(0, len(fpos), 257)))
    _assert_valid(ff.floor, ff.floor_claims, cfg, ring, n_keys)
    offs = {o for o in hu.LOW_OFFSETS + (size - 1,) if o < size}
    assert {int(q) & (size - 1) for q in ff.low} == offs and {0, 15, size - 1} <= offs
    if deep:  # the last quad of the first pass and the first of the second loop, first and last byte
        assert {16 * 63, 16 * 64, 16 * 255 + 15, 16 * 256} <= offs
    got = _assert_oracle([ff.floor], ff.floor_claims, cfg, ring)
    flat = np.concatenate([got[w0 + ((s - w0) & (ring.W - 1))].ravel() for s in range(ring.W)])  # slot order
    mins = flat.reshape(n_sb, size).min(axis=1)
    low_sb = {int(q) >> shift for q in ff.low}
    assert all(mins[j] == (1 if j in low_sb else F if j in set(ff.floored.tolist()) else 0) for j in range(n_sb))
    assert n_sb <= len(offs) or (len(low_sb) == len(offs) and len(ff.floored) > len(low_sb))
    for q in ff.low:  # one low register among F's
        blk = flat[(int(q) >> shift) << shift:][:size]
        assert (blk == 1).sum() == sum(int(x) >> shift == int(q) >> shift for x in ff.low)

    # probe: F - 1, F, F + 1 into every sub-block on registers of their own, 2 into every low register
    ppos = ring.pos(ff.probe_claims[:, 0], ff.probe_claims[:, 1], ff.probe_claims[:, 2])
    assert len(set(ppos)) == len(ppos) == 3 * len(ff.floored) + len(ff.low)
    _assert_scalar(ff.probe, ff.probe_claims, p, pick=range(0, len(ppos), max(1, len(ppos) // 500)))
    assert np.array_equal(hu.claims_of(ff.probe, cfg), ff.probe_claims)
    _assert_valid(ff.probe, ff.probe_claims, cfg, ring, n_keys)
    by_pos = dict(zip(ppos.tolist(), ff.probe_claims[:, 3].tolist()))
    assert all(by_pos[int(q)] == 2 for q in ff.low)
    for j in ff.floored:
        inside = sorted(r for q, r in by_pos.items() if q >> shift == j and q not in set(ff.low.tolist()))
        assert inside == [F - 1, F, F + 1], j
    assert all(by_pos[int(q)] == F + 1 for q in ff.up) and len(ff.up) == len(ff.floored)

    # the bound on hll_filtered, launch by launch, and its registers against the oracle's
    block = 512 if hu.row_of(row)["kernel"] == "small_512" else 1024
    tops = hu.equal_slices(ff.topup, hu.topup_launches(n_sb, block))
    assert len(tops) == 1 + -(-n_sb // (block // 64)) and sum(len(t) for t in tops) == len(ff.topup)
    assert len({-(-len(t) // (2 * block)) for t in tops}) == 1  # one grid for every slice: the rotation has no gaps
    cr = hu.CannotRaise(cfg, w0)
    launches = [ff.floor] + tops + [ff.probe, ff.probe]
    counts = [cr.launch(b) for b in launches]
    assert counts[0] == 0  # one span per register: every one raises
    # a filter whose bounds are all fresh skips the F - 1 and F spans of every sub-block without a low register
    sure = 2 * (len(ff.floored) - len(low_sb))
    assert counts[-2] - counts[-3] >= sure and counts[-1] - counts[-2] == len(ff.probe)
    final = _registers(_oracle(cfg, launches), ring)
    mine = cr.registers()
    for w in final:
        assert np.array_equal(final[w], mine[w]), w
    flat = np.concatenate([final[w0 + ((s - w0) & (ring.W - 1))].ravel() for s in range(ring.W)])
    assert (flat[ff.low] == 2).all() and (flat[ff.up] == F + 1).all()


@pytest.mark.parametrize("row", ["ring_default", "ring_binned", "ring1"])
def test_after_advance_spans(row):
    cfg, n_keys = config_of(row), ALL_ROWS[row]["n_keys"]
    w1 = ring_start(cfg) + 2 * cfg.n_windows
    ring = Ring(cfg, w1)
    geo = hu.filter_geometry(row)
    b, c = hu.after_advance_spans(cfg, w1, n_keys, geo)
    _assert_scalar(b, c, cfg.hll_p, pick=range(0, len(b), 5))
    _assert_valid(b, c, cfg, ring, n_keys)
    assert set(c[:, 3]) == {1, 2}
    pos = ring.pos(c[:, 0], c[:, 1], c[:, 2])
    assert len(set(pos)) == len(pos) == min(3, geo[1]) << geo[0]
    _assert_oracle([b], c, cfg, ring)


def test_rows():
    assert hu.FILTER_ROWS == ("ring_default", "ring_512", "ring_1024_noerr", "ring1", "ring_expo_spec",
                              "ring_expo_generic", "ring_binned", "ring_dense", "p18_lean", "p18_plain", "p18_binned")
    assert [r for r, v in ALL_ROWS.items() if v["lb"] == hu.OFF] == ["p4_lean", "p4_plain", "p4_binned"]
    assert len(ALL_ROWS) == 18
