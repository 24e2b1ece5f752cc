"""What an engine group decides without a device (csrc/sa_shard.h), without a GPU.

Stand-alone programs (their own main, the host compiler, no HIP header, built
plain and with -fsanitize=address,undefined as tests/test_keytable_host.py's;
nothing is preloaded) call the functions spanagg_group.cpp and its partition
kernels call:

  shard   records of (n, count, words): shard_of(w, n, 2^32 % n) per word
  fold    cases of (max_size, members; per member count, zero count, scale,
          offset, buckets): expo_fold over the members in order, the
          accumulator written back the same way

shard_of must equal Python's int % n for every n a group can have (1..64;
kMaxMembers), on every pair of the edge words of a 32-bit half and on drawn
words.  tests/group_util.py's shard_words must land where it says, in the
halves its family names.  The compiled fold of the members' histograms
(pyoracle.expo_series of each member's spans) must be the histogram of the
whole stream, bit for bit, on 1,600 drawn cases of group_util.fold_cases; the
Python restatement agrees, and with each known mistake it disagrees with the
oracle on some case, so the cases can catch what they are there for.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import group_util as gu
import pyoracle
import test_path_decision as tpd

I64, U32, U64 = np.int64, np.uint32, np.uint64
N_CASES = 1600  # every family x max_size x unit ten times over

SHARD_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sa_shard.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  static_assert(sa::kMaxMembers == 64, "the tests walk n = 1..64");
  uint64_t hdr[2];
  while (std::fread(hdr, 8, 2, in) == 2) {
    const uint32_t n = (uint32_t)hdr[0];
    if (n == 0 || n > sa::kMaxMembers) return 4;
    std::vector<uint64_t> w(hdr[1]);
    if (hdr[1] && std::fread(w.data(), 8, w.size(), in) != w.size()) return 5;
    const uint32_t r32 = (uint32_t)((1ULL << 32) % n);
    std::vector<uint32_t> sh(w.size());
    for (size_t i = 0; i < w.size(); ++i) sh[i] = sa::shard_of(w[i], n, r32);
    if (std::fwrite(sh.data(), 4, sh.size(), out) != sh.size()) return 6;
  }
  return std::fclose(out) ? 7 : 0;
}
"""

FOLD_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sa_shard.h"

static bool get(std::FILE *f, int64_t *v, size_t n) { return std::fread(v, 8, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int64_t hdr[2];
  while (get(in, hdr, 2)) {
    const uint32_t max_size = (uint32_t)hdr[0];
    sa::ExpoAcc acc;
    for (int64_t m = 0; m < hdr[1]; ++m) {
      int64_t h[5];  // count, zero count, scale, offset, buckets
      if (!get(in, h, 5)) return 4;
      std::vector<int64_t> raw((size_t)h[4]);
      if (h[4] && !get(in, raw.data(), raw.size())) return 5;
      const std::vector<uint64_t> counts(raw.begin(), raw.end());
      const uint64_t key = 1, count = (uint64_t)h[0], zero = (uint64_t)h[1], sum_ns = 0;
      const double f = 0;
      const int32_t scale = (int32_t)h[2], offset = (int32_t)h[3];
      const uint32_t nb = (uint32_t)h[4];
      sa_exp_result r{};
      r.n_series = 1, r.max_size = max_size;
      r.key_hash = &key, r.count = &count, r.zero_count = &zero, r.sum_ns = &sum_ns;
      r.sum = r.min = r.max = &f;
      r.scale = &scale, r.offset = &offset, r.n_buckets = &nb, r.bucket_counts = counts.data();
      sa::expo_fold(acc, r, 0, max_size);
    }
    std::vector<int64_t> rec = {(int64_t)acc.count, (int64_t)acc.zero, acc.scale, acc.offset, (int64_t)acc.c.size()};
    rec.insert(rec.end(), acc.c.begin(), acc.c.end());
    if (std::fwrite(rec.data(), 8, rec.size(), out) != rec.size()) return 6;
  }
  return std::fclose(out) ? 7 : 0;
}
"""


@pytest.fixture(scope="module", params=[[], tpd.SANITIZE], ids=["plain", "sanitized"])
def programs(request, tmp_path_factory):
    """run(name, request bytes) -> the program's output bytes."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("group")
    flags = list(request.param)
    if flags:  # the sanitizer runtimes linked statically (clang's default; GCC's spelling otherwise)
        gnu = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        flags += ["-static-libasan", "-static-libubsan"] if gnu else ["-static-libsan"]
    with open(os.path.join(tpd.CSRC, "sa_shard.h")) as f:  # the header may not need HIP
        includes = [ln for ln in f if ln.startswith("#include")]
    assert includes and not [ln for ln in includes if "hip" in ln.lower()], includes
    exe = {}
    for name, text in (("shard", SHARD_PROGRAM), ("fold", FOLD_PROGRAM)):
        src, exe[name] = tmp / f"{name}.cpp", tmp / name
        src.write_text(text)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", tpd.CSRC, "-I", tpd.INCLUDE,
                        str(src), "-o", str(exe[name])], check=True)
    count = [0]

    def run(name, data: bytes) -> bytes:
        count[0] += 1
        fin, fout = tmp / f"in{count[0]}", tmp / f"out{count[0]}"
        fin.write_bytes(data)
        subprocess.run([str(exe[name]), str(fin), str(fout)], check=True)
        out = fout.read_bytes()
        os.unlink(fin)
        os.unlink(fout)
        return out

    return run


def _edge_words(n):
    halves = sorted({0, 1, n - 1, n, n + 1, 1 << 16, 1 << 31, (1 << 32) - n, (1 << 32) - 1})
    return [(hi << 32) | lo for hi in halves for lo in halves]


def test_shard_of_is_the_remainder(programs):
    rng = np.random.default_rng(0x5A4D)
    words = {n: np.concatenate([np.array(_edge_words(n), dtype=U64), rng.integers(0, 2**64, 10_000, dtype=U64)])
             for n in range(1, 65)}
    req = b"".join(np.array([n, len(w)], dtype=U64).tobytes() + w.tobytes() for n, w in words.items())
    got = np.frombuffer(programs("shard", req), dtype=U32)
    assert len(got) == sum(len(w) for w in words.values())
    at = 0
    for n, w in words.items():
        want = [x % n for x in w.tolist()]  # Python ints
        assert got[at:at + len(w)].tolist() == want, n
        at += len(w)


@pytest.mark.parametrize("n", [2, 3, 7, 63, 64])
def test_shard_words_land_where_they_say(programs, n):
    rng = np.random.default_rng([n, 0x6A0])
    for dist in gu.DISTS:
        t = gu.targets(n, 4099, dist)
        assert len(t) == 4099 and t.min() >= 0 and t.max() < n
        present = set(t.tolist())
        assert present == {"round_robin": set(range(n)), "skew0": {0, n - 1}, "two_only": {1 % n, n - 1},
                           "one_each": set(range(n))}[dist], dist
        if dist == "skew0":
            assert t[-1] == n - 1 and (t[:-1] == 0).all()
        if dist == "one_each":
            assert [int((t == j).sum()) for j in range(n - 1)] == [1] * (n - 1)
        for family in gu.FAMILIES_W1:
            w = gu.shard_words(n, t, family, rng)
            assert w.dtype == U64 and [x % n for x in w.tolist()] == t.tolist(), (dist, family)
            hi, lo = w >> U64(32), w & U64(gu.TOP32)
            unit = np.gcd((1 << 32) % n, n) == 1  # the high word alone reaches every target
            if family == "low":
                assert not hi.any()
            elif family == "high":
                assert hi.all() and (lo < n).all() and (not unit or not lo.any())
            elif family == "max_hi":
                assert (hi == gu.TOP32).all()
            elif family == "max_lo":
                assert (lo > gu.TOP32 - n).all() and (not unit or (lo == gu.TOP32).all())
            elif family == "near_top":
                assert (w >= U64((1 << 64) - 2 * n)).all()
            else:
                assert len(np.unique(hi)) > 4000 and len(np.unique(lo)) > 4000 // n
            if family != "near_top" and dist == "round_robin":
                assert len(np.unique(w)) > 4099 // 2, family  # drawn, not one word per target
        w = gu.mixed_words(n, t, rng)
        assert [x % n for x in w.tolist()] == t.tolist() and gu.shard_counts(w, n) == [t.tolist().count(j) for j in range(n)]
        assert np.frombuffer(programs("shard", np.array([n, len(w)], dtype=U64).tobytes() + w.tobytes()),
                             dtype=U32).tolist() == t.tolist(), dist


@functools.lru_cache(maxsize=1)
def _cases():
    """The drawn cases with each member's histogram and the whole stream's."""
    out = []
    end = U64(1 << 63)
    for c in gu.fold_cases(0xF01D, N_CASES):
        series = lambda d: pyoracle.expo_series(end - d, np.full(len(d), end), c["max_size"], c["unit_s"])
        members = [series(c["dur"][c["shard"] == i]) for i in range(c["n"])]
        out.append(dict(c, members=members, whole=series(c["dur"])))
    return out


def test_cases_cover_what_they_name():
    cases = _cases()
    seen = {(c["family"], c["max_size"], c["unit_s"]) for c in cases}
    assert len(seen) == len(gu.FAMILIES) * len(gu.MAX_SIZES) * 2
    assert {c["n"] for c in cases} == {2, 3, 4, 5}
    assert all(len(c["dur"]) <= 40 for c in cases)
    scales = lambda c: [m["scale"] for m in c["members"] if len(m["counts"])]
    assert max(max(scales(c)) - min(scales(c)) for c in cases if scales(c)) >= 20  # scales 20 apart in one fold
    assert any(m["offset"] < 0 for c in cases if c["unit_s"] for m in c["members"])
    assert any(m["count"] and not len(m["counts"]) for c in cases if c["family"] == "zero_shard" for m in c["members"])
    assert all(sum(1 for m in c["members"] if m["count"]) == 1 for c in cases if c["family"] == "one_shard")
    assert any(m["count"] == 0 for c in cases for m in c["members"])  # a member that holds nothing of the series


def test_compiled_fold_is_the_whole_stream(programs):
    cases = _cases()
    req = []
    for c in cases:
        req.append(np.array([c["max_size"], c["n"]], dtype=I64))
        for m in c["members"]:
            req.append(np.array([m["count"], m["zero_count"], m["scale"], m["offset"], len(m["counts"])], dtype=I64))
            req.append(m["counts"].astype(I64))
    got = np.frombuffer(programs("fold", b"".join(r.tobytes() for r in req)), dtype=I64)
    at, bad = 0, []
    for i, c in enumerate(cases):
        count, zero, scale, offset, nb = (int(x) for x in got[at:at + 5])
        acc = dict(count=count, zero_count=zero, scale=scale, offset=offset, counts=got[at + 5:at + 5 + nb].tolist())
        at += 5 + nb
        assert nb <= c["max_size"], (i, c["family"])
        if not gu.same_histogram(acc if count else None, c["whole"]):
            bad.append((i, c["family"], c["max_size"], c["unit_s"], acc, c["whole"]))
    assert at == len(got)
    assert not bad, (len(bad), bad[:3])


def test_restated_fold_is_the_whole_stream():
    for i, c in enumerate(_cases()):
        assert gu.same_histogram(gu.fold_all(c["members"], c["max_size"]), c["whole"]), (i, c["family"], c["max_size"])


@pytest.mark.parametrize("wrong", gu.WRONG)
def test_every_known_mistake_shows_on_some_case(wrong):
    seen = [(c["family"], c["max_size"], c["unit_s"]) for c in _cases()
            if not gu.same_histogram(gu.fold_all(c["members"], c["max_size"], wrong), c["whole"])]
    assert seen, wrong
    if wrong == "toward_zero":  # negative indices only: below one unit
        assert any(unit_s for _, _, unit_s in seen)
    if wrong == "no_downscale":
        assert any(M <= 5 for _, M, _ in seen)
