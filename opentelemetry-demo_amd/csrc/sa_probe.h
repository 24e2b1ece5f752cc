// sa_probe.h -- the key tables' probe sequences: which slots a series id may
// occupy, in which order.  Plain C++ (no HIP header): the kernels and the
// flush-time lookups take it through sa_internal.h, and a stand-alone host
// program can call the same functions (tests/test_keytable_host.py).
#pragma once
#include <cstdint>

#include "sa_path.h"  // kPartBinBits

// host/device qualifier: empty under a plain C++ compiler
#if defined(__HIPCC__) || defined(__HIP__)
#define SA_HD __host__ __device__
#else
#define SA_HD
#endif

namespace sa {

// Partitioned HBM-table path: a span's bin is the top kPartBinBits bits of its key
SA_HD inline uint32_t part_bin(uint64_t key) { return (uint32_t)(key >> (64 - kPartBinBits)); }

// ---------------------------------------------------------------------------
// Binned key table (high-cardinality path, spanagg_binned.hip).
// The table of cap = 2^log2cap slots is split into kPartBins bins of
// SB = 2^log2sb slots: a key lives in the bin given by the top kPartBinBits
// bits of m = key * kmul (kmul odd, so the map is a bijection and 0 stays the
// EMPTY marker).  Within the bin the sub-table is buckets of 4 slots with two
// choices, as the small table (probe_seq): positions 0-3 are bucket b1,
// then bucket b2 and the buckets after it in order (wrapping inside the bin),
// so a lookup is two 32-B bucket reads for nearly every key.  One aggregate
// workgroup per bin mirrors the whole sub-table in LDS at the same positions,
// so the bin's keys and counter rows are read and written as one contiguous
// block.
constexpr uint32_t kBinShift = 64 - kPartBinBits;          // bin = m >> kBinShift
struct BtSeq {
  uint32_t b1, b2, nbmask;
};
SA_HD inline BtSeq bt_seq(uint64_t m, uint32_t log2sb) {
  const uint32_t h1 = ((uint32_t)m ^ (uint32_t)(m >> 29)) * 0x9E3779B1u;
  const uint32_t h2 = (h1 ^ (h1 >> 16)) * 0x85EBCA6Bu;
  const uint32_t sh = 34 - log2sb;  // top (log2sb - 2) bits
  return BtSeq{h1 >> sh, h2 >> sh, (1u << (log2sb - 2)) - 1};
}
// in-bin slot of probe position i (i < bt_probe_max: every slot is reached)
SA_HD inline uint32_t bt_pos(const BtSeq &q, uint32_t i) {
  if (i < 4) return q.b1 * 4 + i;
  const uint32_t r = i - 4;
  return ((q.b2 + (r >> 2)) & q.nbmask) * 4 + (r & 3);
}
SA_HD inline uint32_t bt_probe_max(uint32_t log2sb) { return (1u << log2sb) + 4; }
SA_HD inline uint32_t bt_slot(uint64_t m, uint32_t log2sb, uint32_t i) {
  return ((uint32_t)(m >> kBinShift) << log2sb) | bt_pos(bt_seq(m, log2sb), i);
}

// Key-table layout: cap = 2^log2cap slots in buckets of 4 (log2cap in 4..31).
// A key's probe sequence is its first-choice bucket b1, then its second-choice
// bucket b2, then the buckets after b2 in order (every slot within cap + 4
// positions).  Inserts CAS into the first empty slot of the sequence and slots
// never empty again, so concurrent inserts of one key meet at the same slot.
// Two choices keep 97-99 % of a ~0.7-load table's keys in b1/b2, so the LDS
// lookup of the ingest kernel is two fixed 32-B bucket reads with no probe
// loop (ids are xxh64 outputs from the host; any bits are usable).
struct ProbeSeq {
  uint32_t b1, b2, nbmask;
};
SA_HD inline ProbeSeq probe_seq(uint64_t key, uint32_t log2cap) {
  const uint32_t h1 = ((uint32_t)key ^ (uint32_t)(key >> 32)) * 0x9E3779B1u;
  // second choice from a 24-bit multiply (v_mul_u32_u24, full rate; a 32-bit
  // multiply is quarter rate): the top bits of its low word mix all 24 inputs
  const uint32_t h2 = ((h1 ^ (h1 >> 16)) & 0xFFFFFFu) * 0x85EBCAu;
  const uint32_t sh = 34 - log2cap;  // top (log2cap - 2) bits
  return ProbeSeq{h1 >> sh, h2 >> sh, (1u << (log2cap - 2)) - 1};
}
SA_HD inline uint32_t seq_slot(const ProbeSeq &p, uint32_t i) {
  if (i < 4) return p.b1 * 4 + i;
  const uint32_t q = i - 4;
  return ((p.b2 + (q >> 2)) & p.nbmask) * 4 + (q & 3);
}
inline uint32_t max_probe_of(uint32_t log2cap) { return (1u << log2cap) + 4; }

}  // namespace sa
