"""The key tables on adversarial series ids and full tables, against the CPU oracle.

The rest of the suite feeds the open-addressed key tables uniformly random
ids at load <= 0.7, where 97-99 % of the keys sit in their two first-choice
buckets.  Here the ids come from tests/keytable_util.py's families -- found by
inverting the probe hash -- so the lookups of every path walk long chains,
wrap at the table's end, race to insert different keys down one sequence from
many workgroups, meet keys that differ in one half or one bit, and run on
tables that are exactly full and three keys over.  tests/test_keytable_host.py
checks on the CPU that the workloads are what they claim (the families'
sequences by the compiled probe functions, at least 90 % of a chain outside
its b1/b2, the rows' decisions, the oracle's series counts).

Every case first asserts its path, kernel and table through
Engine.debug_geometry() and that its launch spans more than one workgroup.
Bar: RED rows bit-exact (duration sums by parity_util.SUM_RTOL), every ring
window's HLL registers and count-min cells bit-exact, the stats exact,
dropped_table_full 0 unless the case overfills the table.  An overfull table
keeps exactly table_capacity whole series; the dropped ones are whole series
too, their spans counted, and their sketch updates are all there: the HLL
never depended on the key, and an ERROR span without a slot adds to the
count-min cells directly (csrc/sa_device.h sketch_post).
"""
import numpy as np
import pytest

import keytable_util as kt
import pyoracle
from geometry_util import check_against_oracle, expected_oor, ring_start, unit_div
from keytable_util import FULL_ROWS, KT_ROWS, TABLE_ROWS
from parity_util import assert_red_equal
from spanagg import Config, Engine, Group, _lib
from spanagg._lib import OPT_GROUP_COPY

pytestmark = pytest.mark.gpu


def _engine(row):
    cfg = Config(**KT_ROWS[row]["cfg"])
    e = Engine(cfg)
    try:
        g = kt.assert_kt_geometry(e, row)
        assert e.stats()["table_capacity"] == kt.cap_of(row)
        e.window_advance(ring_start(cfg))
    except BaseException:
        e.close()
        raise
    return e, cfg, ring_start(cfg), g


def _workload(rng, row, cfg, g, keys):
    b = kt.workload(rng, kt.spans_for(len(keys)), cfg, keys, ring_start(cfg))
    assert kt.workgroups(row, g, len(b)) > 1  # the inserts race across workgroups
    return b


def _intervals(row, family, variant, ingest=None):
    """The three intervals of a chain case; returns the three flush results."""
    sets, _ = kt.chain_intervals(row, family, variant)
    rng = np.random.default_rng([TABLE_ROWS.index(row), len(family)])
    e, cfg, w0, g = _engine(row)
    out, done = [], []
    with e:
        for keys in sets:
            b = _workload(rng, row, cfg, g, keys)
            (ingest or (lambda e, b: e.ingest(b)))(e, b)
            out.append(check_against_oracle(e, [b], cfg, w0, earlier=done))
            done.append(b)
            # under half the table stays resident (interval 1 of every small row); over half is reclaimed
            assert e.stats()["n_keys"] == kt.resident_after_flush(row, len(keys))
        assert kt.resident_after_flush(row, len(sets[1])) == 0  # intervals 2 and 3: the reclaim happened
        if row != "kt_part17":
            assert kt.resident_after_flush(row, len(sets[0])) == len(sets[0])  # interval 1: nothing reclaimed
    return out


@pytest.mark.parametrize("row", TABLE_ROWS)
def test_chain(row):
    """One sequence over 40 % of the table (kt_part17: 200 chains of 256)."""
    _intervals(row, "one_sequence", None)


@pytest.mark.parametrize("row,variant", [(r, v) for r in TABLE_ROWS for v in kt.wrap_variants(r)])
def test_wrapping_chain(row, variant):
    """The chain's b2 is the table's last bucket: the walk wraps to bucket 0."""
    _intervals(row, "wrapping", variant)


@pytest.mark.parametrize("row", list(KT_ROWS))
def test_halves(row):
    """Keys equal in one half, single-bit neighbours, the edge values: a lookup
    that compares part of a key merges two of these series."""
    keys = kt.halves_keys(row)
    e, cfg, w0, g = _engine(row)
    with e:
        b = kt.workload(np.random.default_rng(len(keys)), kt.spans_for(2 * len(keys)), cfg, keys, w0, per_key=3)
        assert kt.workgroups(row, g, len(b)) > 1
        assert np.unique(b.key_hash[b.key_hash != 0], return_counts=True)[1].min() >= 3
        e.ingest(b)
        check_against_oracle(e, [b], cfg, w0)
        e.ingest(b)  # the keys resident now
        check_against_oracle(e, [b], cfg, w0, earlier=[b])


def _oracle(cfg, batches):
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for b in batches:
        o.ingest(b)
    return o


def _assert_sketches_and_stats(e, o, cfg, w0, batches, dropped):
    seen = set(o.window_ids())
    for wid in range(w0, w0 + cfg.n_windows):
        sk = e.window_read(wid)
        if wid in seen:
            hll, cms = o.window(wid)
            assert np.array_equal(sk.hll, hll), ("hll", wid)
            assert np.array_equal(sk.cms, cms), ("cms", wid)  # slotless ERROR spans included
        else:
            assert not sk.hll.any() and not sk.cms.any(), wid
    st, st_o = e.stats(), o.stats()
    assert st["spans"] == st_o["spans"] == sum(len(b) for b in batches)
    assert st["zero_key"] == st_o["zero_key"]
    assert st["invalid_service"] == st_o["invalid_service"]
    assert st["window_out_of_range"] == expected_oor(batches, cfg, w0)
    assert st["dropped_table_full"] == dropped


def _check_overfull(e, b, cfg, w0, cap):
    """The flush of a table three keys over: SA_EFULL, exactly `cap` rows each
    the oracle's row of its key, the missing keys dropped as whole series,
    every sketch as the oracle's over all spans."""
    o = _oracle(cfg, [b])
    zero = int((b.key_hash == 0).sum())
    if cfg.exp_max_size:
        res = e.flush_exp(allow_drops=True)
        ora = pyoracle.expo_aggregate(b, cfg.exp_max_size, cfg.unit == "s")
        all_keys = np.array(sorted(ora), dtype=np.uint64)
        for i, k in enumerate(res.key_hash):
            r = ora[int(k)]
            assert (int(res.count[i]), int(res.zero_count[i])) == (r["count"], r["zero_count"]), k
            assert (int(res.scale[i]), int(res.offset[i])) == (r["scale"], r["offset"]), k
            assert [int(x) for x in res.buckets[i]] == [int(x) for x in r["counts"]], k
            assert res.min[i] == r["min"] and res.max[i] == r["max"], k
            assert abs(res.sum[i] - r["sum"]) <= 1e-9 * max(abs(r["sum"]), 1e-300), k
        missing = np.setdiff1d(all_keys, res.key_hash)
        dropped = sum(ora[int(k)]["count"] for k in missing)
        kept = int(res.count.sum())
    else:
        res = e.flush(allow_drops=True)
        ora = o.series()
        wrapped = ora["sum_go"] * unit_div(cfg) >= 0.999 * 2.0 ** 64  # (as geometry_util.check_against_oracle)
        ora["sum_go"] = np.where(wrapped, ora["sum_ns"] / unit_div(cfg), ora["sum_go"])
        all_keys = ora["key_hash"]
        pos = np.searchsorted(all_keys, res.key_hash)
        assert (pos < len(all_keys)).all() and np.array_equal(all_keys[pos], res.key_hash)
        assert_red_equal(res, {k: v[pos] for k, v in ora.items()}, unit_div=unit_div(cfg))
        gone = np.ones(len(all_keys), bool)
        gone[pos] = False
        missing, dropped = all_keys[gone], int(ora["calls"][gone].sum())
        kept = int(res.calls.sum())
    assert res.status == _lib.SA_EFULL
    assert len(res.key_hash) == cap == len(np.unique(res.key_hash))
    assert len(missing) == len(all_keys) - cap == 3
    assert kept + dropped + zero == len(b)
    _assert_sketches_and_stats(e, o, cfg, w0, [b], dropped)


FULL_CASES = [(r, w) for r in FULL_ROWS for w in (False, True)]
FULL_IDS = [f"{r}-{'one_chain' if w else 'chain40'}" for r, w in FULL_CASES]


@pytest.mark.parametrize("row,whole", FULL_CASES, ids=FULL_IDS)
def test_exactly_full(row, whole):
    """table_capacity distinct keys, 40 % of them one chain (or all of them:
    then a key sits at the sequence's last position): nothing dropped, every
    row exact, and the flush reclaims the table."""
    e, cfg, w0, g = _engine(row)
    with e:
        keys = kt.full_keys(row, whole=whole)
        assert len(keys) == e.stats()["table_capacity"]
        b = _workload(np.random.default_rng(FULL_ROWS.index(row)), row, cfg, g, keys)
        e.ingest(b)
        res = check_against_oracle(e, [b], cfg, w0)  # raises on SA_EFULL, asserts dropped_table_full == 0
        assert len(res.key_hash) == len(keys) and res.status == 0
        assert e.stats()["n_keys"] == 0


@pytest.mark.parametrize("row,whole", FULL_CASES, ids=FULL_IDS)
def test_three_keys_over(row, whole):
    """table_capacity + 3 distinct keys: SA_EFULL, table_capacity exact rows,
    three whole series dropped and counted, and the sketches of all spans --
    the dropped series' ERROR spans in the count-min cells."""
    e, cfg, w0, g = _engine(row)
    with e:
        keys = kt.full_keys(row, extra=3, whole=whole)
        b = _workload(np.random.default_rng(100 + FULL_ROWS.index(row)), row, cfg, g, keys)
        e.ingest(b)
        _check_overfull(e, b, cfg, w0, kt.cap_of(row))
        assert e.stats()["n_keys"] == 0


@pytest.mark.parametrize("n", [256, 259])
def test_one_bin(n):
    """SA_OPT_IDENTITY_IDS: n keys in one bin of 256 slots, on one sequence that
    wraps inside the bin -- exactly full, then three keys over."""
    row = "kt_binned"
    e, cfg, w0, g = _engine(row)
    with e:
        keys = kt.one_bin_sequence(kt.BINNED_LOG2SB, n)
        b = _workload(np.random.default_rng(n), row, cfg, g, keys)
        e.ingest(b)
        if n == 256:
            res = check_against_oracle(e, [b], cfg, w0)
            assert len(res.key_hash) == 256
        else:
            _check_overfull(e, b, cfg, w0, 256)


def _two_streams(e, b):
    """The batch in two device halves on two streams, no ordering between them."""
    import torch
    dev = torch.device("cuda", 0)
    streams, keep = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)], []
    h = len(b) // 2 & ~3
    for part in (b.slice(0, h), b.slice(h, len(b))):
        keep.append([torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(dev)
                     for c in part.columns()])
    torch.cuda.synchronize(dev)
    for s, cols in zip(streams, keep):
        e.ingest_device(*cols, stream=s.cuda_stream)
    torch.cuda.synchronize(dev)


@pytest.mark.parametrize("row", ["kt_default", "kt_part17"])
def test_concurrent_inserts(row):
    """The chain workload's launches on two streams: both insert down the same
    sequences at once."""
    _intervals(row, "one_sequence", None, ingest=_two_streams)


@pytest.mark.parametrize("row", ["kt_default", "kt_part"])
def test_group_flush_on_chains_and_a_full_member(row):
    """Two members on one device, every key of one chain: member 0's table
    exactly full (so one key sits at the sequence's last position), each
    holding chain keys the other lacks -- the flush gathers every key of the
    union from both (gather_dense_kernel: present keys deep in a chain, absent
    keys against a table without an empty slot)."""
    cfg = Config(**dict(KT_ROWS[row]["cfg"], options=OPT_GROUP_COPY))
    w0 = ring_start(cfg)
    with Engine(cfg) as e:
        g = kt.assert_kt_geometry(e, row)
    sets = kt.group_sets(row)
    b = kt.group_batch(np.random.default_rng(7), cfg, sets, w0)
    assert kt.workgroups(row, g, len(b) // 2) > 1
    m0, m1 = kt.member_keys(b, 0), kt.member_keys(b, 1)
    assert len(m0) == kt.cap_of(row)
    for mine, theirs in ((m0, m1), (m1, m0)):
        assert len(np.setdiff1d(np.intersect1d(mine, sets["chain"]), theirs)) >= 80
    assert len(np.intersect1d(np.intersect1d(m0, m1), sets["chain"])) >= 80
    with Group([0, 0], cfg) as grp:
        grp.window_advance(w0)
        grp.ingest(b)
        res = grp.flush()
        o = _oracle(cfg, [b])
        assert_red_equal(res, o.series(), unit_div=unit_div(cfg))
        seen = set(o.window_ids())
        for wid in range(w0, w0 + cfg.n_windows):
            sk = grp.window_read(wid)
            assert wid in seen
            hll, cms = o.window(wid)
            assert np.array_equal(sk.hll, hll) and np.array_equal(sk.cms, cms), wid
        st, st_o = grp.stats(), o.stats()
        assert st["dropped_table_full"] == 0 and st["spans"] == len(b)
        assert (st["zero_key"], st["invalid_service"]) == (st_o["zero_key"], st_o["invalid_service"])
        assert st["window_out_of_range"] == expected_oor([b], cfg, w0)
        assert st["table_capacity"] == 2 * kt.cap_of(row)
        assert st["n_keys"] == len(m1)  # member 0 reclaimed its full table; member 1, under half, kept its keys


def test_chain_runs_identical():
    a, b = (_intervals("kt_default", "one_sequence", None) for _ in range(2))
    for x, y in zip(a, b):
        for f in ("key_hash", "bucket_counts", "calls", "sum_ns", "sum"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), f
