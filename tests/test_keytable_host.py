"""The key tables' probe sequences and the adversarial key families, without a GPU.

A stand-alone program (its own main, the host compiler, no HIP header, built
plain and with -fsanitize=address,undefined as tests/test_path_decision.py's;
nothing is preloaded) calls the functions of csrc/sa_probe.h the kernels
call.  It reads a binary request (a mode, a range of table sizes, keys) and
writes u32 records:

  mode 0  per log2cap, per key: max_probe_of, b1, b2, nbmask, seq_slot at
          positions 0..11 and at the last four before max_probe
  mode 1  per log2sb, per key: bt_probe_max, b1, b2, nbmask, bt_pos at the same
          positions, part_bin, bt_slot at positions 5 and bt_probe_max - 1
  mode 2  one log2cap, per key: the whole walk, seq_slot at 0 .. max_probe - 1
  mode 3  the same with bt_pos inside a bin

tests/keytable_util.py's NumPy mirror must agree with it on 10^5 random keys
and on every family, for log2cap 4..22 and log2sb 8..11; the families'
properties are asserted on the program's output, not the mirror's.

The chain condition: keys with one sequence own at most 8 slots of their two
first-choice buckets, so of a chain of n keys at least n - 8 lie outside
b1/b2 whatever the insertion order -- at least 90 % from 80 keys on.  Every
chain of every row is that long except kt_min's, whose whole table is 16
slots: there the bound is stated as what it is (n - 8 of at most 16; 90 %
cannot hold in four buckets).  A sequential insertion with the mirror shows
the same and that every workload fits its table.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import keytable_util as kt
import pyoracle
import test_path_decision as tpd
from geometry_util import ring_start
from keytable_util import KT_ROWS, TABLE_ROWS, U32, U64
from spanagg import Config

POSITIONS = list(range(12))
LOG2CAPS, LOG2SBS = range(4, 23), range(8, 12)

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sa_probe.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  uint64_t hdr[4];
  if (std::fread(hdr, 8, 4, in) != 4) return 4;
  const uint64_t mode = hdr[0], lo = hdr[1], hi = hdr[2], n = hdr[3];
  std::vector<uint64_t> keys(n);
  if (n && std::fread(keys.data(), 8, n, in) != n) return 5;
  std::vector<uint32_t> rec;
  for (uint32_t l2 = (uint32_t)lo; l2 <= (uint32_t)hi; ++l2) {
    for (uint64_t k : keys) {
      rec.clear();
      if (mode == 0) {
        const sa::ProbeSeq p = sa::probe_seq(k, l2);
        const uint32_t mp = sa::max_probe_of(l2);
        rec.insert(rec.end(), {mp, p.b1, p.b2, p.nbmask});
        for (uint32_t i = 0; i < 12; ++i) rec.push_back(sa::seq_slot(p, i));
        for (uint32_t i = mp - 4; i < mp; ++i) rec.push_back(sa::seq_slot(p, i));
      } else if (mode == 1) {
        const sa::BtSeq q = sa::bt_seq(k, l2);
        const uint32_t mp = sa::bt_probe_max(l2);
        rec.insert(rec.end(), {mp, q.b1, q.b2, q.nbmask});
        for (uint32_t i = 0; i < 12; ++i) rec.push_back(sa::bt_pos(q, i));
        for (uint32_t i = mp - 4; i < mp; ++i) rec.push_back(sa::bt_pos(q, i));
        rec.insert(rec.end(), {sa::part_bin(k), sa::bt_slot(k, l2, 5), sa::bt_slot(k, l2, mp - 1)});
      } else if (mode == 2) {
        const sa::ProbeSeq p = sa::probe_seq(k, l2);
        for (uint32_t i = 0; i < sa::max_probe_of(l2); ++i) rec.push_back(sa::seq_slot(p, i));
      } else {
        const sa::BtSeq q = sa::bt_seq(k, l2);
        for (uint32_t i = 0; i < sa::bt_probe_max(l2); ++i) rec.push_back(sa::bt_pos(q, i));
      }
      if (std::fwrite(rec.data(), 4, rec.size(), out) != rec.size()) return 6;
    }
  }
  return std::fclose(out) ? 7 : 0;
}
"""


@pytest.fixture(scope="module", params=[[], tpd.SANITIZE], ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """run(mode, lo, hi, keys) -> the program's u32 records, [hi - lo + 1][len(keys)][record]."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("keytable")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    flags = list(request.param)
    if flags:  # the sanitizer runtimes linked statically (clang's default; GCC's spelling otherwise)
        gnu = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        flags += ["-static-libasan", "-static-libubsan"] if gnu else ["-static-libsan"]
    src.write_text(PROGRAM)
    for header in ("sa_probe.h", "sa_path.h"):  # sa_probe.h includes sa_path.h: neither may need HIP
        with open(os.path.join(tpd.CSRC, header)) as f:
            includes = [ln for ln in f if ln.startswith("#include")]
        assert includes and not [ln for ln in includes if "hip" in ln.lower()], includes
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", tpd.CSRC, "-I", tpd.INCLUDE,
                    str(src), "-o", str(exe)], check=True)
    count = [0]

    def run(mode, lo, hi, keys):
        keys = np.ascontiguousarray(keys, dtype=U64)
        count[0] += 1
        fin, fout = tmp / f"in{count[0]}", tmp / f"out{count[0]}"
        with open(fin, "wb") as f:
            f.write(np.array([mode, lo, hi, len(keys)], dtype=U64).tobytes())
            f.write(keys.tobytes())
        subprocess.run([str(exe), str(fin), str(fout)], check=True)
        out = np.fromfile(fout, dtype=U32)
        os.unlink(fin)
        os.unlink(fout)
        return out.reshape(hi - lo + 1, len(keys), -1)

    return run


def _family_keys():
    """Every family at every table size it is built for, as one key list."""
    keys = [kt.EDGES, kt.halves(11), kt.halves(4), kt.halves(17)]
    for L in sorted({r["log2cap"] for r in KT_ROWS.values()} - {19}):
        keys.append(kt.one_sequence(L, 64))
        keys += [kt.wrapping(L, 64, v) for v in kt.WRAP_VARIANTS]
    keys += [kt.one_bin_sequence(sb, 64, wrap=w) for sb in LOG2SBS for w in (False, True)]
    return np.concatenate(keys)


def _mirror_records(keys, log2, binned):
    seq = (kt.bt_seq if binned else kt.probe_seq)(keys, log2)
    mp = kt.max_probe_of(log2)
    pos = POSITIONS + list(range(mp - 4, mp))
    cols = [np.full(len(keys), mp, U32), seq[0], seq[1], np.full(len(keys), seq[2], U32)]
    cols += [kt.seq_slot(seq, i) for i in pos]
    if binned:
        cols += [kt.part_bin(keys), kt.bt_slot(keys, log2, 5), kt.bt_slot(keys, log2, mp - 1)]
    return np.stack(cols, axis=1)


def test_mirror_equals_compiled_functions(probe):
    rnd = np.random.default_rng(0x7AB1E).integers(0, 2**64, 100_000, dtype=U64)
    keys = np.concatenate([rnd, _family_keys()])
    got = probe(0, LOG2CAPS[0], LOG2CAPS[-1], keys)
    assert got.shape == (len(LOG2CAPS), len(keys), 20)
    for j, L in enumerate(LOG2CAPS):
        assert np.array_equal(got[j], _mirror_records(keys, L, False)), L
    got = probe(1, LOG2SBS[0], LOG2SBS[-1], keys)
    assert got.shape == (len(LOG2SBS), len(keys), 23)
    for j, sb in enumerate(LOG2SBS):
        assert np.array_equal(got[j], _mirror_records(keys, sb, True)), sb


def _one_walk(probe, mode, log2, keys):
    """The family's shared (b1, b2) and whole walk, by the compiled functions."""
    rec = probe(mode - 2, log2, log2, keys)[0]
    assert (rec[:, 1] == rec[0, 1]).all() and (rec[:, 2] == rec[0, 2]).all()  # one b1, one b2
    assert len(np.unique(keys)) == len(keys) and (np.asarray(keys) != 0).all()
    walk = probe(mode, log2, log2, keys[:1])[0, 0]
    assert len(walk) == (1 << log2) + 4
    assert np.array_equal(np.unique(walk), np.arange(1 << log2, dtype=U32))  # every slot within cap + 4 positions
    assert np.array_equal(walk[:12], rec[0, 4:16])
    return int(rec[0, 1]), int(rec[0, 2]), walk


@pytest.mark.parametrize("log2cap", sorted({r["log2cap"] for r in KT_ROWS.values()} - {19}))
def test_family_properties(probe, log2cap):
    last = (1 << (log2cap - 2)) - 1
    b1, b2, _ = _one_walk(probe, 2, log2cap, kt.one_sequence(log2cap, 300))
    assert b1 != b2
    for variant in kt.WRAP_VARIANTS:
        b1, b2, walk = _one_walk(probe, 2, log2cap, kt.wrapping(log2cap, 300, variant))
        assert b2 == last and b1 == {"last": b1, "b1_eq_b2": last, "b1_zero": 0}[variant]
        assert (variant != "last") or b1 not in (0, last)
        assert 0 in (walk[:9] >> 2), variant  # bucket 0 by position 8
        assert (walk[4:8] >> 2 == last).all() and walk[8] == 0
    # halves: distinct, non-zero, the edge values present, each group of four in one first-choice bucket
    h = kt.halves(log2cap)
    assert len(np.unique(h)) == len(h) and (h != 0).all() and np.isin(kt.EDGES, h).all()
    assert len(h) >= 16 + 6 + 8 * 64
    rec = probe(0, log2cap, log2cap, h[:16])[0]
    lo, hi = h[:16] & U64(0xFFFFFFFF), h[:16] >> U64(32)
    for g in range(4):
        s = slice(4 * g, 4 * g + 4)
        assert (rec[s, 1] == rec[4 * g, 1]).all(), g
        same, other = (lo, hi) if g < 2 else (hi, lo)
        assert len(np.unique(same[s])) == 1 and len(np.unique(other[s])) == 4, g


@pytest.mark.parametrize("log2sb", LOG2SBS)
def test_one_bin_sequence(probe, log2sb):
    for wrap in (False, True):
        keys = kt.one_bin_sequence(log2sb, 259, wrap=wrap)
        b1, b2, walk = _one_walk(probe, 3, log2sb, keys)
        rec = probe(1, log2sb, log2sb, keys)[0]
        assert (rec[:, 20] == rec[0, 20]).all()  # one bin
        assert (rec[:, 21] >> log2sb == rec[0, 20]).all()  # bt_slot lies in it
        if wrap:
            assert b2 == (1 << (log2sb - 2)) - 1 and b1 != b2 and walk[8] == 0


def _insert(keys, log2cap, binned=False):
    """Sequential find-or-insert of `keys` in order with the mirror (inside one
    bin if binned): each key's probe position, -1 without a slot.  Slots of a
    bucket fill in order, so a fill count per bucket stands for the slots."""
    nb = 1 << (log2cap - 2)
    fill = [0] * nb
    b1s, b2s, _ = (kt.bt_seq if binned else kt.probe_seq)(keys, log2cap)
    pos_of = np.full(len(keys), -1)
    for j, (b1, b2) in enumerate(zip(b1s.tolist(), b2s.tolist())):
        if fill[b1] < 4:
            pos_of[j] = fill[b1]
            fill[b1] += 1
            continue
        for k in range(nb):
            b = (b2 + k) & (nb - 1)
            if fill[b] < 4:
                pos_of[j] = 4 * (k + 1) + fill[b]
                fill[b] += 1
                break
    return pos_of


def _chain_cases(row):
    for family, variant in [("one_sequence", None)] + [("wrapping", v) for v in kt.wrap_variants(row)]:
        sets, chains = kt.chain_intervals(row, family, variant)
        for keys, cs in zip(sets[:2], chains):
            assert len(keys) <= kt.cap_of(row) and np.isin(np.concatenate(cs), keys).all()
            yield keys, cs


@pytest.mark.parametrize("row", TABLE_ROWS)
def test_chain_condition(probe, row):
    """At least n - 8 of each chain's n keys lie outside b1/b2 in any order
    (one b1, one b2, at most 8 slots, by the compiled functions): 90 % from 80
    keys on."""
    L, cap = KT_ROWS[row]["log2cap"], kt.cap_of(row)
    for keys, chains in _chain_cases(row):
        rec = probe(0, L, L, np.concatenate(chains))[0]
        at = 0
        for c in chains:
            r = rec[at:at + len(c)]
            at += len(c)
            assert (r[:, 1] == r[0, 1]).all() and (r[:, 2] == r[0, 2]).all()
            in_buckets = len({int(s) for s in r[0, 4:12]})  # the slots of b1 and b2: 8, or 4 when b1 == b2
            assert in_buckets in (4, 8)
            if cap > 16:
                assert len(c) >= 80 and len(c) - in_buckets >= 0.9 * len(c), (row, len(c))
            else:  # kt_min: 16 slots in four buckets -- the bound itself
                assert len(c) <= 16
    if row in kt.FULL_ROWS:
        for whole in (False, True):
            chain = kt.one_sequence(L, kt.full_chain_len(row, whole), 0)
            for extra in (0, 3):
                keys = kt.full_keys(row, extra, whole)
                assert len(keys) == cap + extra == len(np.unique(keys))
                assert np.isin(chain, keys).all() and 4 * len(chain) >= cap
    if row in ("kt_default", "kt_part"):
        s = kt.group_sets(row)
        assert len(s["only0"]) + len(s["both"]) == cap
        for part in ("only0", "both", "only1"):
            assert np.isin(s["chain"], s[part]).sum() >= 80, part


@pytest.mark.parametrize("row", [r for r in TABLE_ROWS if r != "kt_part17"])
def test_workloads_fit_and_leave_the_buckets(row):
    """One sequential insertion with the mirror, in a shuffled order: every
    chain workload fits its table with all but 8 keys of the chain past
    position 7, and a full table holds exactly table_capacity keys."""
    L, cap, rng = KT_ROWS[row]["log2cap"], kt.cap_of(row), np.random.default_rng(5)
    for keys, chains in _chain_cases(row):
        keys = rng.permutation(keys)
        pos = _insert(keys, L)
        assert (pos >= 0).all()
        for c in chains:
            deep = int((pos[np.isin(keys, c)] >= 8).sum())
            assert deep >= len(c) - 8 and (cap == 16 or deep >= 0.9 * len(c))
    if row in kt.FULL_ROWS:
        for extra, whole in ((0, False), (3, False), (0, True), (3, True)):
            pos = _insert(rng.permutation(kt.full_keys(row, extra, whole)), L)
            assert (pos < 0).sum() == extra
            assert not whole or pos.max() == cap + 3  # one chain over the table: a key at position max_probe - 1
    if row in ("kt_default", "kt_part"):
        s = kt.group_sets(row)
        pos = _insert(rng.permutation(np.concatenate([s["only0"], s["both"]])), L)
        assert pos.min() >= 0 and pos.max() == cap + 3  # member 0: full, a key at the last position


def test_one_bin_fits_exactly():
    sb = kt.BINNED_LOG2SB
    assert (_insert(kt.one_bin_sequence(sb, 256), sb, binned=True) >= 0).all()
    pos = _insert(kt.one_bin_sequence(sb, 259), sb, binned=True)
    assert (pos < 0).sum() == 3 and (pos >= 8).sum() == 248


def test_rows_decide_as_stated(tmp_path):
    """KT_ROWS through tests/test_path_decision.py's program and assertions."""
    cxx = shutil.which("c++") or shutil.which("g++")
    src, exe = tmp_path / "path_decision.cpp", tmp_path / "path_decision"
    src.write_text(tpd.PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", tpd.CSRC, "-I", tpd.INCLUDE, str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], input="".join(tpd._line(**r["cfg"]) for r in KT_ROWS.values()),
                         capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(ln.split()) for ln in out if ln]
    assert len(got) == len(KT_ROWS)
    tpd._assert_rows(KT_ROWS, got)
    assert kt.cap_of("kt_min") == 16 and kt.cap_of("kt_part") == 4096 and kt.cap_of("kt_binned") >> 11 == 256


def _series(cfg, batch):
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(batch)
    return o.series()


@pytest.mark.parametrize("row", list(KT_ROWS))
def test_oracle_series_counts(row):
    """The oracle alone: every workload holds exactly its keys, each with two
    spans or more, 10 % ERROR spans and 1 % without a key."""
    cfg, rng = Config(**KT_ROWS[row]["cfg"]), np.random.default_rng(11)
    sets = []
    if row == "kt_binned":
        sets = [kt.one_bin_sequence(kt.BINNED_LOG2SB, n) for n in (256, 259)]
    else:
        sets += kt.chain_intervals(row)[0][:2] + [kt.chain_intervals(row, "wrapping", v)[0][1] for v in kt.wrap_variants(row)]
        sets.append(kt.halves_keys(row))
        if row in kt.FULL_ROWS:
            sets += [kt.full_keys(row, x, w) for w in (False, True) for x in (0, 3)]
    for keys in sets:
        b = kt.workload(rng, kt.spans_for(len(keys)), cfg, keys, ring_start(cfg))
        ora = _series(cfg, b)
        assert np.array_equal(ora["key_hash"], np.sort(keys))
        assert int(ora["calls"].min()) >= 2 and int(ora["calls"].sum()) == int((b.key_hash != 0).sum())
        err = ((b.meta >> 19) & 3) == 2
        assert 0.08 < err.mean() < 0.12 and 0.005 < (b.key_hash == 0).mean() < 0.02
        hot = np.isin(b.key_hash, keys[:8]).mean()
        assert hot > 0.3  # the hot head: half the spans, less what moved (keytable_util.workload)
    if row in ("kt_default", "kt_part"):
        s = kt.group_sets(row)
        b = kt.group_batch(rng, cfg, s, ring_start(cfg))
        m0, m1 = kt.member_keys(b, 0), kt.member_keys(b, 1)
        assert np.array_equal(m0, np.sort(np.concatenate([s["only0"], s["both"]]))) and len(m0) == kt.cap_of(row)
        assert np.array_equal(m1, np.sort(np.concatenate([s["only1"], s["both"]])))
        assert len(_series(cfg, b)["key_hash"]) == len(m0) + len(s["only1"])
