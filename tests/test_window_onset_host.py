"""sa_window_latency_onset without a GPU: the plain-Python rule
(spanagg.sketch.latency_onset) against the numpy restatement of
tests/onset_util.py on the GPU tests' workloads, what those workloads can tell
apart, the crafted case's hand-written answers, the C-ABI's declarations, and
the new argument rule of csrc/sa_query_args.h through a stand-alone program (its
own main, host compiler, no HIP header), plain and built with
-fsanitize=address,undefined (nothing is preloaded).

The argument cases' answers are written from include/spanagg.h's text:

  onset    k in 1..SA_TOP_MAX_K (4,096); flag bits other than SA_ONSET_FALL (1)
           are refused; threshold_ns given: q_ppm must be 0; threshold_ns null:
           q_ppm in 1..10^6
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import onset_util as ou
import spanagg
from spanagg import _lib, sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opentelemetry-demo_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def test_sketch_equals_the_restatement():
    for what, p, mc, _, fall, _ in ou.every_pairs():
        stride = 37 if p.shape[0] == 1000 else 1  # (the rule does not depend on the service)
        for s in range(0, p.shape[0], stride):
            assert sketch.latency_onset(p[s].tolist(), mc, fall) == ou.split(p[s], mc, fall), (what, s)


def test_sketch_rule_on_small_rows():
    rise = sketch.latency_onset(ou.CRAFTED_PAIRS)
    assert rise == (3, 26_700, 445_000, 200, 1, 300, 135)
    assert sketch.latency_onset(ou.CRAFTED_PAIRS, 200) == rise and sketch.latency_onset(ou.CRAFTED_PAIRS, 201) is None
    assert sketch.latency_onset(ou.CRAFTED_PAIRS, fall=True)[:2] == (5, -8_900)
    assert sketch.latency_onset(ou.CRAFTED_PAIRS[::-1], fall=True)[:3] == (4, 26_700, 445_000)
    assert sketch.latency_onset([(10, 1)] * 6)[:3] == (5, 0, 0)  # D == 0 everywhere: the latest split
    assert sketch.latency_onset([(5, 1)]) is None and sketch.latency_onset([]) is None
    assert sketch.latency_onset([(0, 0), (5, 1)]) is None and sketch.latency_onset([(5, 1), (5, 1)], 0)[0] == 1
    big = 1 << 43
    assert sketch.latency_onset([(big, 0), (big - 1, big - 1)])[1] == big * (big - 1)  # (past 2^63: Python's integers)


def test_the_crafted_case_as_the_issue_states_it():
    c = ou.case("crafted")
    w0 = c.w0
    rise, at200, at201, fall, one_window, d_eq, d_above, d_never = (ou.want("crafted", j) for j in range(8))
    for w in (rise, at200, d_eq):
        assert (w.n_services, w.n_eligible, w.n_matched, w.spans) == (1, 1, 1, 500)
        assert w.services.tolist() == [0] and w.onset_window.tolist() == [w0 + 3] and w.delta_ppm.tolist() == [445_000]
        assert (w.total_before.tolist(), w.slow_before.tolist()) == ([200], [1])
        assert (w.total_after.tolist(), w.slow_after.tolist()) == ([300], [135]) and w.d == [26_700]
        assert w.threshold_bin.tolist() == [100] and w.effective_ns.tolist() == [ou.su.CRAFTED_THRESHOLD]
    p = ou.pairs(c.ref, c.cfg, c.calls[0], ou.thresholds(c.ref, c.cfg, c.calls[0]))
    assert p[0].tolist() == [list(v) for v in ou.CRAFTED_PAIRS]
    d = lambda t: ou.split(np.concatenate([p[0, :t].sum(0, keepdims=True), p[0, t:].sum(0, keepdims=True)]))[1]
    assert d(2) == d(3) == 26_700  # the tie across the empty window goes to the later split
    assert (at201.n_eligible, at201.n_matched, len(at201.services)) == (0, 0, 0)
    assert (fall.n_eligible, fall.n_matched) == (1, 0) and ou.split(p[0], 1, True)[1] == -8_900
    assert (one_window.n_eligible, one_window.n_matched, one_window.spans) == (0, 0, 100)  # no split
    assert (d_above.n_eligible, d_above.n_matched) == (1, 0) and (d_never.n_eligible, d_never.n_matched) == (1, 0)
    rev = ou.want("crafted_rev", 3)
    assert rev.onset_window.tolist() == [w0 + 4] and rev.delta_ppm.tolist() == [445_000] and rev.fall
    assert (rev.total_before.tolist(), rev.slow_before.tolist()) == ([300], [135])
    flat = ou.want("crafted_flat", 0)
    assert (flat.n_eligible, flat.n_matched, flat.spans) == (1, 0, 60)
    fp = ou.case("crafted_flat")
    fpairs = ou.pairs(fp.ref, fp.cfg, fp.calls[0], ou.thresholds(fp.ref, fp.cfg, fp.calls[0]))
    assert fpairs[0].tolist() == [[10, 1]] * 6 and ou.split(fpairs[0])[:2] == (5, 0)


def test_the_workloads_hit_their_targets():
    c = ou.case("every_bin")
    w = ou.want("every_bin", 0)  # the given thresholds: service s at bin s
    assert w.n_eligible == 256 and w.n_matched == 255 and w.spans == 2 * 256 * 256
    assert w.services.tolist() == list(range(255))  # 255 - s slow spans of 256: the order is the id's
    assert w.threshold_bin.tolist() == list(range(255)) and w.slow_after.tolist() == [255 - s for s in range(255)]
    assert set(w.total_before.tolist()) == {256} and not w.slow_before.any() and set(w.onset_window.tolist()) == {c.w0 + 1}
    for j, b in enumerate(ou.EVERY_BIN_POOLED, 1):  # the pooled thresholds: every service at bin b
        tb = ou.thresholds(c.ref, c.cfg, c.calls[j])
        assert tb.tolist() == [b] * 256, (j, b)
        assert ou.want("every_bin", j).n_matched == (256 if b < 255 else 0)
    assert {3, 4, 63, 64, 251, 252, 255} <= set(ou.EVERY_BIN_POOLED)
    lg = ou.case("lengths")
    assert sorted({call.last - call.first + 1 for call in lg.calls}) == [1, 2, 64, 65, 127, 128]
    full = ou.want("lengths", 10)  # 128 windows, the pooled threshold
    assert full.services.tolist()[0] == 0 and abs(int(full.onset_window[0]) - (lg.w0 + 40)) <= 1
    assert ou.want("lengths", 12).services.tolist()[0] == 1  # the fall: service 1, at window 70
    assert abs(int(ou.want("lengths", 12).onset_window[0]) - (lg.w0 + 70)) <= 1
    assert ou.want("lengths", 0).n_eligible == 0 and ou.want("lengths", 2).n_eligible > 0  # 1 window; 2 windows
    for S in (64, 129, 1000):  # n_matched above k and below it
        assert ou.want(f"services{S}", 1).n_matched > 10 and ou.want(f"services{S}", 2).n_matched < _lib.TOP_MAX_K
        assert len(ou.want(f"services{S}", 2).services) == ou.want(f"services{S}", 2).n_matched > 10
    big = ou.probe("big")
    assert max(ou.want_probe("big", 0).d) > 1 << 80 and ou.want_probe("big", 0).n_matched == 5  # (service 5: delta_ppm 0)
    assert (1 << 44) - 16 < int(big.pairs[5, :, 0].sum(dtype=object)) < 1 << 44
    assert ou.probe("random200").pairs.shape == (70, 200, 2)
    t = ou.want_probe("ties", 0)
    assert t.services.tolist()[:3] == [5, 4, 6] and t.delta_ppm.tolist()[:3] == [500_000] * 3  # count, then id
    assert t.n_eligible == 7 and t.delta_ppm[t.services.tolist().index(3)] == 166_667


def _every_answer(wrong=None):
    for name in ou.CASES:
        c = ou.case(name)
        for j, call in enumerate(c.calls):
            if c.cfg.n_services == 1000 and wrong:
                continue  # (the rule does not depend on the service count)
            yield (name, j), ou.expected(c.ref, c.cfg, call, wrong) if wrong else ou.want(name, j)
    for name in ou.PROBES:
        c = ou.probe(name)
        for j, call in enumerate(c.calls):
            yield (name, j), ou.expected_probe(c.pairs, *call.args(), wrong=wrong) if wrong else ou.want_probe(name, j)


def _differs(a, b):
    return any(getattr(a, f) != getattr(b, f) for f in ou.SCALARS) or any(
        not np.array_equal(getattr(a, f), getattr(b, f)) for f in ou.FIELDS)


@pytest.mark.parametrize("wrong", ou.WRONG)
def test_every_known_mistake_shows_on_some_workload(wrong):
    right = dict(_every_answer())
    seen = [what for what, bad in _every_answer(wrong) if _differs(right[what], bad)]
    assert seen, wrong
    crafted = {"ge_bin": ("crafted", "every_bin"), "first_tie": ("crafted", "ties"), "d_i64": ("big",),
               "one_sided_min": ("crafted", "ties"), "edge_split": ("crafted", "lengths"), "unfloored": ("ties",)}[wrong]
    assert [w for w in seen if w[0] in crafted], (wrong, seen)
    if wrong == "d_i64":  # another split and another order, as the probe test needs
        a, b = ou.want_probe("big", 0), ou.expected_probe(ou.probe("big").pairs, *ou.probe("big").calls[0].args(), wrong=wrong)
        assert a.services.tolist() != b.services.tolist() and sorted(a.services.tolist()) == sorted(b.services.tolist())
        assert dict(zip(a.services.tolist(), a.splits)) != dict(zip(b.services.tolist(), b.splits))


def test_declarations():
    lib = _lib.load()
    header = open(os.path.join(INCLUDE, "spanagg.h")).read()
    diag = open(os.path.join(INCLUDE, "spanagg_diag.h")).read()
    for sym in ("sa_window_latency_onset", "sa_group_window_latency_onset", "sa_onset_result_free"):
        assert hasattr(lib, sym) and re.search(r"\b%s\(" % sym, header), sym
    assert hasattr(lib, "sa_onset_probe") and re.search(r"\bsa_onset_probe\(", diag) and "sa_onset_probe" not in header
    assert "#define SA_ONSET_FALL 1u" in header
    assert _lib.SA_ONSET_FALL == spanagg.SA_ONSET_FALL == 1
    # two u64, four u32, five u64, nine pointers
    assert C.sizeof(_lib.sa_onset_result) == 2 * 8 + 4 * 4 + 5 * 8 + 9 * C.sizeof(C.c_void_p) == 144
    assert [f for f, _ in _lib.sa_onset_result._fields_] == [
        "first_window", "last_window", "k", "n", "flags", "q_ppm", "min_count", "n_services", "n_eligible", "n_matched",
        "spans", "services", "onset_window", "delta_ppm", "threshold_bin", "effective_ns", "total_before", "slow_before",
        "total_after", "slow_after"]
    assert "#define SA_OPT_ALL           0x7FFu" in header and "#define SA_ABI_VERSION 4" in header
    assert lib.sa_abi_version() == _lib.ABI_VERSION == 4
    assert {"OnsetResult", "SA_ONSET_FALL"} <= set(spanagg.__all__)
    out = C.POINTER(_lib.sa_onset_result)()
    assert lib.sa_window_latency_onset(None, 0, 0, 1, 500_000, None, 1, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    assert lib.sa_group_window_latency_onset(None, 0, 0, 1, 500_000, None, 1, 1, 0, C.byref(out)) == _lib.SA_EINVAL
    pair = (C.c_uint64 * 2)(1, 0)
    assert lib.sa_onset_probe(None, pair, 1, 1, 1, 1, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    lib.sa_onset_result_free(None)


def _onset(k, q_ppm, given, flags=0):
    return f"onset {k} {q_ppm} {int(given)} {flags}"


# (the line the program reads, what it must print)
ARG_CASES = [
    # ---- onset: k, q_ppm, whether threshold_ns is given, flags
    (_onset(1, 500_000, False), "ok"), (_onset(4096, 1, False), "ok"), (_onset(10, 1_000_000, False), "ok"),
    (_onset(10, 0, True), "ok"), (_onset(10, 0, True, 1), "ok"), (_onset(10, 950_000, False, 1), "ok"),  # SA_ONSET_FALL
    (_onset(0, 500_000, False), "bad"), (_onset(4097, 500_000, False), "bad"),   # k outside 1..SA_TOP_MAX_K
    (_onset(10, 0, False), "bad"), (_onset(10, 1_000_001, False), "bad"),        # pooled: q_ppm outside 1..10^6
    (_onset(10, 1, True), "bad"), (_onset(10, 950_000, True), "bad"),            # given: q_ppm must be 0
    (_onset(10, 500_000, False, 2), "bad"), (_onset(10, 0, True, 3), "bad"),     # flag bits other than SA_ONSET_FALL
    (_onset(10, 500_000, False, 1 << 31), "bad"),
]

PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "sa_query_args.h"

int main() {
  std::string rule;
  while (std::cin >> rule) {
    if (rule != "onset") return 2;
    unsigned k, q, given, flags;
    std::cin >> k >> q >> given >> flags;
    if (!std::cin) return 3;
    const uint64_t thresholds[1] = {1000};
    std::puts(sa_args::onset_args(k, q, given ? thresholds : nullptr, flags) ? "bad" : "ok");
  }
  return 0;
}
"""

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_argument_rules(tmp_path, flags):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "onset_args.cpp", tmp_path / "onset_args"
    if flags:  # the sanitizer runtimes linked statically (clang's default; GCC's spelling otherwise)
        gnu = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        flags = flags + (["-static-libasan", "-static-libubsan"] if gnu else ["-static-libsan"])
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", INCLUDE,
                    str(src), "-o", str(exe)], check=True)
    lines = "".join(line + "\n" for line, _ in ARG_CASES)
    run = subprocess.run([str(exe)], input=lines, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(ARG_CASES), (len(got), len(ARG_CASES))
    wrong = [(line, want, g) for (line, want), g in zip(ARG_CASES, got) if g != want]
    assert not wrong, wrong
