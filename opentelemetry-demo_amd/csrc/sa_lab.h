// sa_lab.h -- the engine's laboratory knobs.  The SPANAGG_AB build (`make ab`
// -> libspanagg_ab.so, used by tools/ for A/B runs and ablations) fills them
// from the environment; the product library holds a constexpr object of
// defaults and reads no environment at all.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

struct LabKnobs {
  // per engine: sa_create takes a fresh reading (lab_for_create) and keeps what
  // it needs in the engine (tools/ switch these between engines of one process)
  uint32_t slab_sets = 0;    // SPANAGG_SLAB_SETS: slab sets, 1..4 (0: the default)
  bool xstream = false;      // SPANAGG_XSTREAM=1: the histogram kernels on an engine stream
  bool kmul_set = false;     // SPANAGG_KMUL: the binned path's id multiplier, fixed
  uint64_t kmul = 0;
  uint32_t xidx = 1;         // SPANAGG_XIDX_OFF: IngestParams::xidx 2, or 3 for "2" (ablation: results wrong)
  // per process, read once (lab)
  bool ev_sys = false;       // SPANAGG_EV_SYS=1: ordering events with the default (system-scope) release
  long fail_agg = 0;         // SPANAGG_FAIL_AGG=n: the n-th aggregate launch of the process fails
  int xrec = -1;             // SPANAGG_XREC=0 / 1 / 2: the exponential slab path's span words
  uint32_t xc_diag = 0;      // SPANAGG_XC_DIAG: ExpoParams::diag
  bool xt = true;            // SPANAGG_XT=0: the counting kernel's tail through HBM atomics
  bool bt_pipe = true;       // SPANAGG_BT_PIPE=0: each aggregate after its scatter, on the caller's stream
  bool bt_pair = true;       // SPANAGG_BT_PAIR=0: every launch aggregated alone
  bool no_setev = false;     // SPANAGG_NO_SETEV: no slab-set event (one stream only; prices the event)
};

#ifdef SPANAGG_AB
inline const char *ab_env(const char *name) { return std::getenv(name); }
inline bool ab_is(const char *name, bool zero) {  // set, and zero / non-zero as asked
  const char *v = ab_env(name);
  return v && (std::atoi(v) == 0) == zero;
}
inline LabKnobs lab_read() {
  LabKnobs k;
  if (const char *v = ab_env("SPANAGG_SLAB_SETS")) k.slab_sets = (uint32_t)std::max(1, std::min(4, std::atoi(v)));
  k.xstream = ab_is("SPANAGG_XSTREAM", false);
  if (const char *v = ab_env("SPANAGG_KMUL")) k.kmul_set = true, k.kmul = std::strtoull(v, nullptr, 0);
  if (const char *v = ab_env("SPANAGG_XIDX_OFF")) k.xidx = std::atoi(v) == 2 ? 3 : 2;
  k.ev_sys = ab_is("SPANAGG_EV_SYS", false);
  if (const char *v = ab_env("SPANAGG_FAIL_AGG")) k.fail_agg = std::atol(v);
  if (const char *v = ab_env("SPANAGG_XREC")) k.xrec = std::atoi(v);
  if (const char *v = ab_env("SPANAGG_XC_DIAG")) k.xc_diag = (uint32_t)std::strtoul(v, nullptr, 0);
  k.xt = !ab_is("SPANAGG_XT", true);
  k.bt_pipe = !ab_is("SPANAGG_BT_PIPE", true);
  k.bt_pair = !ab_is("SPANAGG_BT_PAIR", true);
  k.no_setev = ab_env("SPANAGG_NO_SETEV") != nullptr;
  return k;
}
inline const LabKnobs &lab() {
  static const LabKnobs knobs = lab_read();
  return knobs;
}
inline LabKnobs lab_for_create() { return lab_read(); }
#else
inline constexpr LabKnobs kLabDefaults{};
constexpr const LabKnobs &lab() { return kLabDefaults; }
constexpr LabKnobs lab_for_create() { return kLabDefaults; }
#endif
