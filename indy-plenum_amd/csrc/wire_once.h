// wire_once.h -- the work list of a scanned wire batch: which items the verify
// kernels run over, and which item's verdict every other item takes
// (edverify.h edv_wire_verify_list).
//
// Compiled for the device (edv_wire_once_*_kernel, edverify.hip: one lane per
// item) and for the host (host_check.cpp hc_wire_once, wire_corpus_check.cpp:
// the same code run serially in any item order, every read and write asserted
// in bounds).
//
// select.  Item i is LIVE iff status[i] == 0, uidx[i] < nu and
// kid_u[uidx[i]] != kOnceSkip; its group is keyed (a registered key id) or
// general (kOnceNoId: the key's 32 bytes travel with the item).  Every other
// item is dead: its bit stays 0 and nothing of it is read.
//
// insert (only when each distinct (identifier, signature, message) is to be
// verified once).  The table is wire_idents.h's: open addressing, linear
// probing, `cap` slots (a power of two; the device uses cap >= 2 n), two uint32
// arrays set to kIdentEmpty beforehand, owner[s] an ITEM INDEX whose triple the
// slot stands for and first[s] the smallest index among the items that
// resolved to the slot.  The scan finished every signature, span and message
// byte before this code starts, so a slot's key can be read through its owner
// as soon as the owner is visible.  The same argument as wire_idents.h's gives
// one slot per triple in any arrival order, and both atomics are tested first
// with relaxed loads for the same reason (copies arrive roughly in index order
// and almost every one finds its owner and a smaller first[]).
//
// The probe is BOUNDED: after `probe` slots (the device: kWireOnceProbe) a lane
// stops and the item is its own representative.  Correctness never depends on
// the table -- an item without a slot is verified by itself, an item with one
// takes the verdict of an item with the same identifier index, signature and
// message bytes, which the verify kernels would have treated identically.  A
// flood of items with equal signatures and different messages therefore costs
// at most `probe` compares per item and one verify each.  The slots a lane
// passes are occupied and contiguous, and the set of occupied slots does not
// depend on the order of arrival, so a table whose longest run of occupied
// slots is below the bound has no give-ups in any order.
//
// The hash covers the sixteen aligned 32-bit words of the signature, the
// identifier index and the message length: the signature alone separates
// everything but a forger's copies.  Equality is the identifier index, the
// sixteen words, the length, then the message bytes; the two messages sit at
// unrelated alignments in the batch, so they are compared eight bytes at a
// time through the accessor's word64(pos) -- an eight-byte little-endian read
// that is correct at ANY byte position -- and byte by byte for the last < 8.
//
// flag / rank / emit, per group: flag[i] = live, in the group and its own
// representative; rank = the exclusive sum of the flags over n + 1 entries
// (rank[n] = m, the group's lanes); wo_emit_* writes representative i's
// signature, span pair and key at position rank[i] of the group's contiguous
// inputs.  scatter: wo_bit reads the representative's bit from its group's
// result words.
#pragma once
#include <stdint.h>

#include "wire_idents.h"

namespace edv {

constexpr uint32_t kWireOnceProbe = 128;  // slots a device lane passes before it gives up
constexpr uint32_t kOnceNoId = 0xffffffffu;  // edverify.h EDV_WIRE_NO_ID
constexpr uint32_t kOnceSkip = 0xfffffffeu;  // edverify.h EDV_WIRE_SKIP
constexpr uint32_t kOnceDead = 0, kOnceKeyed = 1, kOnceGeneral = 2;  // an item's group

// select: the item's group.
template <class St, class U, class K>
EDV_WI_HD uint32_t wo_group(St status, U uidx, K kid_u, uint32_t nu, uint64_t i) {
  if (status[i] != 0) return kOnceDead;
  const uint32_t u = uidx[i];
  if (u >= nu) return kOnceDead;
  const uint32_t k = kid_u[u];
  return k == kOnceSkip ? kOnceDead : k == kOnceNoId ? kOnceGeneral : kOnceKeyed;
}

// The item's message span lies inside the `bytes` bytes the messages live in.
template <class Sp>
EDV_WI_HD bool wo_span_ok(Sp ms, Sp me, uint64_t bytes, uint64_t i) {
  return ms[i] <= me[i] && me[i] <= bytes && me[i] - ms[i] <= 0xffffffffull;
}

template <class Sg, class U>
EDV_WI_HD uint64_t wo_hash(Sg sigw, U uidx, uint32_t len, uint64_t i) {
  uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)uidx[i] << 32 | len);
  for (uint32_t k = 0; k < 16; ++k) h = (h ^ (uint64_t)sigw[16 * i + k]) * 0x100000001b3ull;
  h ^= h >> 32;
  h *= 0xd6e8feb86659fd93ull;
  h ^= h >> 32;
  return h;
}

// Items a and b (live, wo_span_ok) have the same identifier index, signature and message.
template <class Sg, class Sp, class M, class U>
EDV_WI_HD bool wo_same(Sg sigw, Sp ms, Sp me, M msg, U uidx, uint64_t a, uint64_t b) {
  if (uidx[a] != uidx[b]) return false;
  for (uint32_t k = 0; k < 16; ++k)
    if (sigw[16 * a + k] != sigw[16 * b + k]) return false;
  const uint64_t len = me[a] - ms[a];
  if (me[b] - ms[b] != len) return false;
  const uint64_t pa = ms[a], pb = ms[b];
  uint64_t k = 0;
  for (; k + 8 <= len; k += 8)
    if (msg.word64(pa + k) != msg.word64(pb + k)) return false;
  for (; k < len; ++k)
    if (msg[pa + k] != msg[pb + k]) return false;
  return true;
}

// Live item i into the table: its slot, or kIdentEmpty when `probe` slots (or all of them) were
// passed -- the item then stands for itself.  Tab as wi_insert's.
template <class Sg, class Sp, class M, class U, class Tab>
EDV_WI_HD uint32_t wo_insert(Sg sigw, Sp ms, Sp me, M msg, U uidx, Tab tab, uint32_t cap, uint32_t probe, uint32_t i) {
  const uint32_t steps = probe < cap ? probe : cap;
  uint32_t s = (uint32_t)wo_hash(sigw, uidx, (uint32_t)(me[i] - ms[i]), i) & (cap - 1);
  for (uint32_t step = 0; step < steps; ++step, s = (s + 1) & (cap - 1)) {
    uint32_t o = tab.owner_load(s);
    if (o == kIdentEmpty) {
      o = tab.owner_cas(s, i);
      if (o == kIdentEmpty) o = i;
    }
    if (o != i && !wo_same(sigw, ms, me, msg, uidx, (uint64_t)i, (uint64_t)o)) continue;
    if (i < tab.first_load(s)) tab.first_min(s, i);
    return s;
  }
  return kIdentEmpty;
}

// After every insert: the item whose verdict item i takes (itself without a slot).
template <class L, class Fi>
EDV_WI_HD uint32_t wo_rep(L slot, Fi first, uint64_t i) {
  const uint32_t s = slot[i];
  return s != kIdentEmpty ? first[s] : (uint32_t)i;
}

// flag: item i is a lane of group g.
template <class G, class L, class Fi>
EDV_WI_HD uint32_t wo_flag(G grp, L slot, Fi first, uint32_t g, uint64_t i) {
  return grp[i] == g && wo_rep(slot, first, i) == (uint32_t)i ? 1u : 0u;
}

// emit: representative i (wo_flag) to position j = rank[i] < m of its group's inputs: the
// signature's sixteen words, the span pair (starts [m] then ends [m]).
template <class Sg, class Sp, class So, class Po>
EDV_WI_HD void wo_emit(Sg sigw, Sp ms, Sp me, uint64_t i, uint64_t j, uint64_t m, So sig_out, Po spans_out) {
  for (uint32_t k = 0; k < 16; ++k) sig_out[16 * j + k] = sigw[16 * i + k];
  spans_out[j] = ms[i];
  spans_out[m + j] = me[i];
}

// scatter: item i's verdict -- its representative's bit in its group's result words (rank_k /
// words_k the keyed group's, rank_g / words_g the general one's); 0 for a dead item.
template <class G, class L, class Fi, class R, class W>
EDV_WI_HD uint32_t wo_bit(G grp, L slot, Fi first, R rank_k, R rank_g, W words_k, W words_g, uint64_t i) {
  const uint32_t g = grp[i];
  if (g == kOnceDead) return 0;
  const uint32_t r = wo_rep(slot, first, i);
  const uint32_t j = g == kOnceKeyed ? rank_k[r] : rank_g[r];
  const uint64_t w = g == kOnceKeyed ? words_k[j >> 6] : words_g[j >> 6];
  return (uint32_t)(w >> (j & 63)) & 1u;
}

}  // namespace edv
