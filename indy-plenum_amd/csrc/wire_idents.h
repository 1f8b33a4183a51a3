// wire_idents.h -- the distinct identifiers of a scanned wire batch and, per
// item, its index into them: what plenum_amd/_hostpack wire_idents computes on
// the host, over the data edv_wire_scan left in HBM.
//
// Compiled for the device (edv_wire_ident_*_kernel, edverify.hip: one lane per
// item) and for the host (host_check.cpp hc_wire_idents: the same code run
// serially in any item order, every read and write asserted in bounds).
//
// Item i (status 0) has the identifier text[off[i] + span[2i] ..][: span[2i+1]]
// -- raw text bytes: the scanner's grammar sends an identifier with a backslash
// to the host, so the bytes are the value.
//
// The table: open addressing, linear probing, `cap` slots (a power of two; the
// device uses cap >= 2 n, so it never fills), two uint32 arrays set to
// kIdentEmpty beforehand:
//   owner[s]   an ITEM INDEX whose identifier the slot stands for.  The slot's
//              key is read from the text through that index; the text was
//              finished by the scan kernel before this code starts, so there is
//              no "tag visible before its payload" window.
//   first[s]   the smallest index among the items that resolved to the slot.
// wi_insert probes from hash & (cap - 1): an empty slot is claimed with a
// compare-and-swap, a slot whose owner has the same bytes is the item's, any
// other slot is passed.  The owner is whichever item of the identifier won the
// swap -- arrival order -- but the slot it won is the first free one of the
// probe chain at that time and every later item of the identifier walks the
// same chain past the same (never emptied) slots, so one identifier has one
// slot.  What comes out -- first[] per identifier, and from it the numbering in
// first-occurrence order -- does not depend on the order of arrival.
//
// Every atomic is tested first.  A batch has about a thousand identifiers for a
// million items, so an unconditional swap or minimum per item would put a
// million atomics on a thousand addresses; items arrive roughly in index order
// and almost every one finds a non-empty owner and a smaller first[] and issues
// no atomic.  The test reads are relaxed atomic loads (never hoisted, served
// from L2) and may be stale, harmlessly:
//   owner   a slot never returns to empty, so a stale EMPTY only costs a
//           compare-and-swap that fails and returns the true owner;
//   first   only decreases, so a stale value is never smaller than the true
//           one: a needed minimum is never skipped, an unneeded one may be done.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EDV_WI_HD __host__ __device__ __forceinline__
#else
#define EDV_WI_HD inline
#endif

namespace edv {

constexpr uint32_t kIdentEmpty = 0xffffffffu;  // an empty slot; slot[i] of an item without one

// FNV-1a over the bytes, then a 64-bit finalizer (the low bits pick the slot).
template <class T>
EDV_WI_HD uint64_t wi_hash(T text, uint64_t at, uint32_t len) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t k = 0; k < len; ++k) h = (h ^ (uint64_t)text[at + k]) * 0x100000001b3ull;
  h ^= h >> 32;
  h *= 0xd6e8feb86659fd93ull;
  h ^= h >> 32;
  return h;
}

// The identifier's span lies inside its item (off is the n + 1 text offsets).
template <class F, class S>
EDV_WI_HD bool wi_span_ok(F off, S span, uint64_t i) {
  return (uint64_t)span[2 * i] + (uint64_t)span[2 * i + 1] <= off[i + 1] - off[i];
}

template <class T>
EDV_WI_HD bool wi_same(T text, uint64_t a, uint64_t b, uint32_t len) {
  for (uint32_t k = 0; k < len; ++k)
    if (text[a + k] != text[b + k]) return false;
  return true;
}

// Item i (status 0, wi_span_ok) into the table: its slot, or kIdentEmpty when
// every slot was passed (cap smaller than the number of identifiers).
// Tab: owner_load(s), owner_cas(s, i) -> the owner before (kIdentEmpty: i won),
// first_load(s), first_min(s, i).
template <class T, class F, class S, class Tab>
EDV_WI_HD uint32_t wi_insert(T text, F off, S span, Tab tab, uint32_t cap, uint32_t i) {
  const uint64_t at = off[i] + span[2 * (uint64_t)i];
  const uint32_t len = span[2 * (uint64_t)i + 1];
  uint32_t s = (uint32_t)wi_hash(text, at, len) & (cap - 1);
  for (uint32_t step = 0; step < cap; ++step, s = (s + 1) & (cap - 1)) {
    uint32_t o = tab.owner_load(s);
    if (o == kIdentEmpty) {
      o = tab.owner_cas(s, i);
      if (o == kIdentEmpty) o = i;
    }
    if (o != i) {
      if (span[2 * (uint64_t)o + 1] != len) continue;
      if (!wi_same(text, at, off[o] + span[2 * (uint64_t)o], len)) continue;
    }
    if (i < tab.first_load(s)) tab.first_min(s, i);
    return s;
  }
  return kIdentEmpty;
}

// After every insert: item i is its identifier's first occurrence.
template <class L, class Fi>
EDV_WI_HD uint32_t wi_flag(L slot, Fi first, uint64_t i) {
  const uint32_t s = slot[i];
  return s != kIdentEmpty && first[s] == (uint32_t)i ? 1u : 0u;
}

// rank = the exclusive prefix sum of the flags over n + 1 entries (rank[n] = nu,
// the number of identifiers): item i's index, nu for an item without a slot.
template <class L, class Fi, class R>
EDV_WI_HD uint32_t wi_index(L slot, Fi first, R rank, uint64_t n, uint64_t i) {
  const uint32_t s = slot[i];
  return s != kIdentEmpty ? rank[first[s]] : rank[n];
}

}  // namespace edv
