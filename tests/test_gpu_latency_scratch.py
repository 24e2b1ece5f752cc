"""The latency queries share one engine's scratch (sa_engine::Latency: one
buffer a role -- sel, thr, pairs, prefix, range_sums, counts, cand, rec and the
ranked rows -- whoever asks): every query in turn on ONE engine, between them
calls that grow the shared buffers and leave them laid out for other services
and other ranges.  Each answer must equal the query's own numpy restatement
(tests/slo_util.py, onset_util.py, latency_movers_util.py, latency_util.py)
and, bit for bit, the same call on a freshly created engine fed the same
batch.  A query that read what another one left -- a buffer it did not grow,
or filled for another layout -- fails one of the two.

5 services on 16 windows (onset_util's shifted workload: three services'
latency moves inside the ring).  The probe's 70 services x 9 windows lie above
the 64-element floor of the growing buffers and above the engine's 5 services,
so thr, pairs, cand and rec all grow between the engine's own calls.
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import latency_movers_util as lmu
import latency_util as lu
import onset_util as ou
import slo_util as su
from geometry_util import ring_start
from spanagg import Engine, Group
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

pytestmark = pytest.mark.gpu

# test_gpu_group.py's transports: two members on device 0 merge through device
# copies; a group of one that asks for RCCL all-reduces for real
TRANSPORTS = [([0, 0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True)]
QUANTILES = (0.5, 0.9, 0.99)


@functools.lru_cache(maxsize=1)
def _case():
    cfg = su._cfg(5, 16)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"latency_scratch"))
    batch = ou._shifted(cfg, w0, 16, rng, 60, {0: (6, 8.0), 1: (10, 0.2), 3: (4, 5.0)})
    steps = [(w0, batch)]
    return SimpleNamespace(cfg=cfg, w0=w0, steps=steps, ref=lu.window_hists(cfg, steps),
                           probe=np.ascontiguousarray(ou.probe("random200").pairs[:, :9]))


@functools.lru_cache(maxsize=1)
def _steps():
    """(name, the call on an engine or a group, what it must return, the
    comparison), in the order they run; the expectations computed once."""
    c = _case()
    w0, last, ref, cfg = c.w0, c.w0 + 15, c.ref, c.cfg
    thr5 = (250_000, int(lu.BIN_HI[150]), 1_000_000, 127, 20_000_000)
    slo3 = su.Call(w0 + 3, last, (2, 4), (100_000, 300_000), (1_000_000, 127, 20_000_000), (4, 0, 2), 5)
    slo5 = su.Call(w0 + 6, last, (7, 1, 3), (50_000, 400_000, 200_000), thr5, None, 20)
    pooled = ou.Call(w0, last, 5, 0.9, None, 20)
    given = ou.Call(w0 + 1, last - 1, 3, 0.0, thr5, 10)
    rise = ((w0, w0 + 5), (w0 + 8, last), 5, (900_000, 500_000), 10, 1, False)
    fall = ((w0 + 1, w0 + 7), (w0 + 9, last - 1), 4, (500_000,), 1, 1, True)
    lat = (w0 + 2, last - 1)
    assert c.probe.shape[:2] == (70, 9) and max(slo3.widths) != max(slo5.widths)
    return (
        ("slo of 3 services", lambda x: x.window_slo(*slo3.args()), su.expected(ref, cfg, slo3), su.assert_slo),
        ("probe 70 x 9", lambda x: x.onset_probe(c.probe, 12, 1 << 20), ou.expected_probe(c.probe, 12, 1 << 20), ou.assert_onset),
        ("latency movers", lambda x: lmu.run(x, rise), lmu.expected(ref, cfg, *rise), lmu.assert_latency_movers),
        ("onset pooled", lambda x: x.window_latency_onset(*pooled.args()), ou.expected(ref, cfg, pooled), ou.assert_onset),
        ("onset given", lambda x: x.window_latency_onset(*given.args()), ou.expected(ref, cfg, given), ou.assert_onset),
        ("slo of 5 services", lambda x: x.window_slo(*slo5.args()), su.expected(ref, cfg, slo5), su.assert_slo),
        ("latency movers fall", lambda x: lmu.run(x, fall), lmu.expected(ref, cfg, *fall), lmu.assert_latency_movers),
        ("latency hist", lambda x: x.window_latency(*lat, None, QUANTILES, True),
         lu.expected(ref, cfg, lat[1], lat[1], lat[1] - lat[0] + 1, None, QUANTILES), lu.assert_latency),
    )


def _loaded(cls, *a):
    c = _case()
    x = cls(*a)
    try:
        for base, batch in c.steps:
            x.window_advance(base)
            x.ingest(batch)
    except BaseException:
        x.close()
        raise
    return x


def _same_bits(a, b, what):
    """Two results of one dataclass, bit for bit."""
    assert type(a) is type(b), what
    for f in dataclasses.fields(a):
        va, vb = getattr(a, f.name), getattr(b, f.name)
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), (what, f.name)
        else:
            assert va == vb, (what, f.name, va, vb)


def _run_in_turn(x, skip=()):
    c = _case()
    ran = 0
    for name, call, want, check in _steps():
        if name in skip:
            continue
        got = call(x)
        check(got, want, name)
        with _loaded(Engine, c.cfg) as fresh:  # (no earlier query's scratch)
            _same_bits(got, call(fresh), name)
        ran += 1
    return ran


def test_every_query_in_turn_on_one_engine():
    c = _case()
    with _loaded(Engine, c.cfg) as e:
        assert _run_in_turn(e) == 8
    # the answers are not empty ones: services matched and rows returned in every ranked query, alerts and burns in the SLO's
    want = {name: w for name, _, w, _ in _steps()}
    assert len(want["probe 70 x 9"].services) == 12 and want["probe 70 x 9"].n_services == 70
    assert len(want["latency movers"].services) >= 1 and len(want["latency movers fall"].services) >= 1
    assert len(want["onset pooled"].services) >= 2 and len(want["onset given"].services) >= 2
    assert want["slo of 3 services"].burning.any() and want["slo of 5 services"].burning.any()
    assert want["slo of 5 services"].total.shape == (10, 3, 5) and want["latency hist"][0].sum() > 1000


@pytest.mark.parametrize("devices,option,rccl", TRANSPORTS, ids=["copy", "rccl"])
def test_every_query_in_turn_on_one_group(devices, option, rccl):
    """The same through a group (without the probe, which is an engine's): its
    member 0 runs every finish in its own scratch, behind its own exports."""
    c = _case()
    with _loaded(Group, devices, dataclasses.replace(c.cfg, options=c.cfg.options | option)) as g:
        assert g.size == len(devices) and g.uses_rccl == rccl
        assert _run_in_turn(g, skip=("probe 70 x 9",)) == 7
