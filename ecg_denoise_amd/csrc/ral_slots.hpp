// The slot protocol of the stream pools (ral_pool_*, ral_newrale_pool_*, ral_rate_pool, ral_beat_pool, ral_rhythm_pool), once
// for all of them: what a table row says about its slot, checked on the host and carried out on the device.
//
// A slot keeps the last hist_len samples of its stream in one of two planes, hist (2, capacity, leads, hist_len).  Every row
// type (include/ralenet.h) names the same seven fields: the stream had n0 samples and gets the c of its chunk, which starts
// x_off samples per lead into the packed chunks; `slot`, which no other row of the table names; `turn`, the plane the row
// reads, samples [n0 - hist_len, n0).  A row that stays open has T = -1 and RAL_POOL_KEEP in flags, and the call writes the
// last hist_len samples received to the OTHER plane, zeros below sample 0; a row that ends has T = n0 + c and no flag, and
// nothing is written for it.  No workgroup reads a plane that another one writes; the host flips the turn of the kept rows.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/ralenet.h"
#include "ral_device.hpp"

// the rules on the shared fields that differ between the pools: the smallest length a stream may end with, whether an open row
// must bring samples, and the wording of the two rules that name a pool's own fields
struct SlotRules {
  long long t_min;
  bool open_needs_chunk;
  const char* range_rule;
  const char* t_rule;
};

struct SlotNoRule {
  template <typename Row> const char* operator()(const Row&) const { return nullptr; }
};

// The host walk over a table, before anything reaches the device: a wrong row would send a kernel out of bounds.  -> null, or
// the rule that is broken with *bad the row that breaks it (-1 if none does).  Per row, in this order: the slot, in_range(row)
// (false: rules.range_rule), turn, flags, T against flags, early(row), the chunk inside the x_total samples per lead that are
// packed (not if x_total < 0: a call without chunks), own(row).  early and own return null or the pool's rule the row breaks.
template <typename Row, typename InRange, typename Early, typename Own>
static const char* slots_walk(const Row* tab, int rows, long long cap, long long x_total, const SlotRules& rules, InRange in_range,
                              Early early, Own own, int* bad) {
  std::vector<bool> seen((size_t)cap, false);
  for (int r = 0; r < rows; ++r) {
    const Row& t = tab[r];
    *bad = r;
    if (t.slot < 0 || t.slot >= cap) return "0 <= slot < capacity";
    if (seen[(size_t)t.slot]) return "every slot at most once";
    seen[(size_t)t.slot] = true;
    if (!in_range(t)) return rules.range_rule;
    if (t.turn != 0 && t.turn != 1) return "turn 0 or 1";
    if (t.flags & ~(RAL_POOL_KEEP)) return "flags RAL_POOL_KEEP or 0";
    const bool keep = (t.flags & RAL_POOL_KEEP) != 0;
    if (t.T >= 0 ? (t.T < rules.t_min || t.T != t.n0 + t.c || keep) : (t.T != -1 || !keep || (rules.open_needs_chunk && t.c < 1)))
      return rules.t_rule;
    if (const char* why = early(t)) return why;
    if (x_total >= 0 && (t.x_off < 0 || t.x_off + t.c > x_total)) return "the chunk inside the packed chunks";
    if (const char* why = own(t)) return why;
  }
  *bad = -1;
  return nullptr;
}

// the table to the device, on the stream of the launches that read it -> 0, or -2 if the copy could not be queued
template <typename Row>
static int slots_upload(const Row* tab, long long rows, Row* tab_dev, hipStream_t s) {
  return hipMemcpyAsync(tab_dev, tab, (size_t)rows * sizeof(Row), hipMemcpyHostToDevice, s) == hipSuccess ? 0 : -2;
}

// where the history of (turn, slot, lead) starts in hist
RAL_DEV size_t slot_plane(int turn, long long slot, long long cap, int leads, int hist_len, int lead = 0) {
  return ((((size_t)turn * cap + slot) * leads) + lead) * hist_len;
}

// Sample `pos` of lead `lead` of a stream of N samples, clamped to [0, N - 1].  The stream is history ++ chunk: lead l's samples
// [n0, N) at chunk + l * chunk_stride, its samples [n0 - hist_len, n0) at hist + l * hist_len.  A record is the stream that has
// received nothing before: hist null, n0 = 0.  (What lies before the history reads the oldest sample kept; the callers' host
// checks see to it that no such value is used.)
RAL_DEV float slot_sample(const float* chunk, long long chunk_stride, const float* hist, int hist_len, long long n0, long long N,
                          int lead, long long pos) {
  pos = pos < 0 ? 0 : (pos > N - 1 ? N - 1 : pos);
  if (pos >= n0) return chunk[lead * chunk_stride + (pos - n0)];
  const long long hi = hist_len - (n0 - pos);
  return hist[(size_t)lead * hist_len + (hi < 0 ? 0 : hi)];
}

// The calling workgroup writes the next history of one (row, lead) that stays open: dst[0, hist_len) = samples
// [n0 + c - hist_len, n0 + c), from hr (the current plane, [n0 - hist_len, n0)) and chunk ([n0, n0 + c)); zeros below sample 0.
RAL_DEV void slot_write_history(const float* hr, const float* chunk, float* dst, long long n0, int c, int hist_len) {
  const long long first = n0 + c - hist_len;       // the stream position of dst[0]
  for (int l = threadIdx.x; l < hist_len; l += blockDim.x) {
    const long long v = (long long)c + l;
    dst[l] = first + l < 0 ? 0.f : (v < hist_len ? hr[v] : chunk[v - hist_len]);
  }
}
