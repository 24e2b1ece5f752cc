"""Dense series indices (SA_OPT_DENSE_IDS), the parts that need no GPU: the
host dictionary spanagg.dense.DenseIds and the configuration checks sa_create
makes before it touches a device."""
import numpy as np
import pytest

from spanagg import Config, DenseIds, Engine, SpanAggError
from spanagg import _lib
from spanagg._lib import OPT_DENSE_IDS, OPT_PARTITIONED
from spanagg.dense import NO_INDEX


def test_option_bit_and_signature():
    assert OPT_DENSE_IDS == 1 << 9
    assert "sa_bind_ids" in [n for n, _, _ in _lib.SIGNATURES]
    assert hasattr(_lib.load(), "sa_bind_ids")


def test_round_trip():
    d = DenseIds(1 << 19)
    h = np.array([0xDEADBEEF, 7, 0xDEADBEEF, 2**64 - 1, 7], dtype=np.uint64)
    ids, ni, nh = d.encode(h)
    assert ids.dtype == np.uint64 and len(ids) == len(h)
    assert [d.hash_of(int(i)) for i in ids] == [int(x) for x in h]
    assert [d.index_of(int(x)) for x in h] == [int(i) for i in ids]
    assert ids[0] == ids[2] and ids[1] == ids[4] and len(set(ids.tolist())) == 3
    assert [d.hash_of(int(i)) for i in ni] == nh.tolist()
    # a second batch: known hashes keep their index and are not reported as new
    ids2, ni2, nh2 = d.encode(np.array([7, 99], dtype=np.uint64))
    assert ids2[0] == ids[1] and nh2.tolist() == [99] and ni2.tolist() == [int(ids2[1])]
    assert len(d) == 4
    assert d.index_of(12345) == 0 and d.hash_of(400_000) == 0


def test_hash_zero_is_id_zero():
    d = DenseIds(16)
    ids, ni, nh = d.encode(np.array([0, 5, 0], dtype=np.uint64))
    assert ids.tolist() == [0, 1, 0]
    assert ni.tolist() == [1] and nh.tolist() == [5]
    assert d.index_of(0) == 0 and d.hash_of(0) == 0


def test_indices_assigned_in_order_of_appearance():
    d = DenseIds(1 << 19)
    ids, ni, nh = d.encode(np.array([900, 3, 900, 500, 3, 1], dtype=np.uint64))
    assert ids.tolist() == [1, 2, 1, 3, 2, 4]
    assert ni.tolist() == [1, 2, 3, 4] and nh.tolist() == [900, 3, 500, 1]
    ids, ni, nh = d.encode(np.array([77, 900], dtype=np.uint64))
    assert ids.tolist() == [5, 1] and ni.tolist() == [5]


def test_exhaustion_gives_the_sentinel():
    d = DenseIds(4)  # indices 1, 2, 3
    ids, ni, nh = d.encode(np.array([10, 20, 30, 40, 10, 40], dtype=np.uint64))
    assert ids.tolist() == [1, 2, 3, NO_INDEX, 1, NO_INDEX]
    assert NO_INDEX == 2**64 - 1
    assert ni.tolist() == [1, 2, 3] and nh.tolist() == [10, 20, 30]
    assert d.index_of(40) == 0 and len(d) == 3


def test_released_index_is_reused_only_after_flushed():
    d = DenseIds(4)
    d.encode(np.array([10, 20, 30], dtype=np.uint64))
    d.release([20])
    assert d.index_of(20) == 0 and d.hash_of(2) == 0
    ids, ni, _ = d.encode(np.array([40], dtype=np.uint64))
    assert ids.tolist() == [NO_INDEX] and len(ni) == 0  # index 2 is not assignable yet
    d.flushed()
    ids, ni, nh = d.encode(np.array([40, 10], dtype=np.uint64))
    assert ids.tolist() == [2, 1] and ni.tolist() == [2] and nh.tolist() == [40]
    assert d.hash_of(2) == 40


def _create_code(**kw):
    with pytest.raises(SpanAggError) as x:
        Engine(Config(n_services=1, **kw))
    return x.value.code


@pytest.mark.parametrize("kw", [
    dict(exp_max_size=160),
    dict(bounds=tuple(float(i + 1) for i in range(18))),
    dict(n_windows=2048),
    dict(options=OPT_DENSE_IDS | OPT_PARTITIONED),
    dict(key_capacity=4_000_000),  # 5 M slots at 1.25 x: 2^23
], ids=["expo", "18-bounds", "2048-windows", "partitioned", "table-above-2^22"])
def test_config_rejected_without_a_device(kw):
    """Each is SA_EINVAL from validate_config, before a device is looked for
    (a valid dense configuration on a machine without a GPU is SA_EDEVICE)."""
    cfg = dict(key_capacity=300_000, n_windows=16, options=OPT_DENSE_IDS)
    cfg.update(kw)
    assert _create_code(**cfg) == _lib.SA_EINVAL


def test_bounds_the_bin_table_cannot_hold_are_rejected():
    # three thresholds between two powers of two (1.1, 1.2, 1.3 ms)
    assert _create_code(key_capacity=300_000, options=OPT_DENSE_IDS, bounds=(1.1, 1.2, 1.3)) == _lib.SA_EINVAL


def test_group_create_rejects_the_option():
    from spanagg import Group
    with pytest.raises(SpanAggError) as x:
        Group([0], Config(n_services=1, key_capacity=300_000, options=OPT_DENSE_IDS))
    assert x.value.code == _lib.SA_EINVAL
