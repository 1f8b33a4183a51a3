// key_dedup.h -- general path, distinct keys of a sub-batch: the table kernel decodes each
// distinct 32-byte key once (a batch of 1M requests from 1,000 signers builds 1,000 tables, not
// 1M).  Open-addressing hash table over the sub-batch: slot = request index of the key's
// representative (0xffffffff = empty); the full 32 bytes are compared, so distinct keys never
// share a table whatever their hash.  Which request becomes the representative depends on the
// order of the atomics; the table -- a function of the key bytes only -- does not.
//
// The bodies of edv_dedup_insert_kernel and edv_dedup_assign_kernel (edverify.hip), shared with
// the probe kernels of tests/native/ed_probe.hip and their CPU twin edv_host_ed_dedup
// (csrc/host_check.cpp).  The device build takes the slots with atomics; the host build runs the
// requests one after the other with plain loads and stores.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fe25519.h"

namespace edv {

constexpr uint32_t kEmptySlot = 0xffffffffu;
constexpr int kDedupBlock = 256;  // lanes per block of the two kernels (edverify.hip kBlock)

// Every key word counts: a family of keys that differs in one word only spreads over the slots
// like any other (each word has its own odd multiplier; words 2, 5 and 3, 7 share one, so a
// single changed word still changes the product).  The hash is fixed and unseeded: keys crafted
// against it can still share a home slot, and the full compare keeps them apart.
EDV_HD uint32_t key_hash(const uint32_t pk[8]) {
  uint32_t h = pk[0] * 0x9e3779b1u;
  h ^= pk[1] * 0x85ebca77u;
  h ^= (pk[2] ^ pk[5]) * 0xc2b2ae3du;
  h ^= (pk[3] ^ pk[7]) * 0x27d4eb2fu;
  h ^= pk[4] * 0x165667b1u;
  h ^= pk[6] * 0xfd7046c5u;
  return h ^ (h >> 15);
}

// the 8 words of request a's key (pk32 is 16-byte aligned: 32-byte records)
EDV_HD void load_key(uint32_t pk[8], const uint8_t* __restrict__ pk32, uint64_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s = (const uint4*)(pk32 + 32 * a);
  for (int k = 0; k < 2; ++k) {
    uint4 v = s[k];
    pk[4 * k] = v.x;
    pk[4 * k + 1] = v.y;
    pk[4 * k + 2] = v.z;
    pk[4 * k + 3] = v.w;
  }
#else
  memcpy(pk, pk32 + 32 * a, 32);
#endif
}

EDV_HD bool same_key(const uint8_t* __restrict__ pk32, uint64_t a, const uint32_t pk[8]) {
  uint32_t w[8];
  load_key(w, pk32, a);
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) eq = eq && w[k] == pk[k];
  return eq;
}

// slot of request i's key (inserting i as the representative if new)
EDV_HD uint32_t dedup_slot(const uint8_t* __restrict__ pk32, uint64_t i, uint32_t* __restrict__ slots,
                           uint32_t nslots, bool insert) {
  uint32_t pk[8];
  load_key(pk, pk32, i);
  uint32_t h = key_hash(pk) % nslots;
  for (uint32_t probe = 0; probe < nslots; ++probe) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t s = __atomic_load_n(&slots[h], __ATOMIC_RELAXED);
#else
    uint32_t s = slots[h];
#endif
    if (s == kEmptySlot) {
      if (!insert) return kEmptySlot;  // unreachable after the insert pass
#if defined(__HIP_DEVICE_COMPILE__)
      s = atomicCAS(&slots[h], kEmptySlot, (uint32_t)i);
#else
      slots[h] = (uint32_t)i;
#endif
      if (s == kEmptySlot) return h;
    }
    if (s == (uint32_t)i || same_key(pk32, s, pk)) return h;
    h = h + 1 == nslots ? 0 : h + 1;
  }
  return kEmptySlot;  // table full: impossible with nslots = 2n
}

// every request records its key's slot
EDV_HD void dedup_insert(const uint8_t* __restrict__ pk32, uint64_t i, uint32_t* __restrict__ slots, uint32_t nslots,
                         uint32_t* __restrict__ req_slot) {
  req_slot[i] = dedup_slot(pk32, i, slots, nslots, true);
}

// representative -> compact key index u (reps[u] = its request)
EDV_HD void dedup_assign(uint64_t i, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ req_slot,
                         uint32_t* __restrict__ slot_u, uint32_t* __restrict__ reps, uint32_t* __restrict__ count) {
  const uint32_t h = req_slot[i];
  if (slots[h] == (uint32_t)i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t u = atomicAdd(count, 1u);
#else
    const uint32_t u = (*count)++;
#endif
    slot_u[h] = u;
    reps[u] = (uint32_t)i;
  }
}

// Tables per distinct key: K = 8 with at least 16 requests per distinct key
// in the sub-batch, K = 4 with at least 4, else 1.  The K tables of all keys
// then fit the sub-batch's scratch (K * count <= n), and the 256 (K-1)/K
// extra doublings per key cost at most 256 (K-1)/K^2 per request against
// 256 (K-1)/K saved in every ladder.  Decided on the device from the
// distinct-key count, identically by the table and ladder kernels.
EDV_HD int split_of(uint32_t count, uint64_t n) {
  return 16ull * count <= n ? 8 : 4ull * count <= n ? 4 : 1;
}

}  // namespace edv
