// node_split_wave_host.h -- TEST INFRASTRUCTURE, host only: the wave of edv_node_split_count_kernel
// and edv_node_split_emit_kernel (edverify.hip) emulated on the CPU over the same lane functions
// (node_split_lanes.h): 64 lanes one after the other, the Hillis-Steele composition the shuffles
// do, the same carry from step to step.  T: t[i] = byte i of the entry (host_check.cpp asserts
// every index, the sanitizer corpus runner reads a heap block of the entry's exact size).
#pragma once
#include <assert.h>
#include <string.h>

#include "node_split_lanes.h"

namespace edv {

inline void wave_scan_maps(uint32_t v[kNslLanes]) {  // inclusive
  for (uint32_t d = 1; d < kNslLanes; d <<= 1) {
    uint32_t o[kNslLanes];
    memcpy(o, v, sizeof o);
    for (uint32_t lane = d; lane < kNslLanes; ++lane) v[lane] = nsl_compose(o[lane - d], v[lane]);
  }
}
inline void wave_scan_sums(uint64_t v[kNslLanes]) {  // inclusive
  for (uint32_t d = 1; d < kNslLanes; d <<= 1) {
    uint64_t o[kNslLanes];
    memcpy(o, v, sizeof o);
    for (uint32_t lane = d; lane < kNslLanes; ++lane) v[lane] = o[lane - d] + v[lane];
  }
}

// One step of the wave at q: the lanes' bytes, and each lane's true state on entry from carry;
// returns the state after the step.
template <class T>
uint32_t wave_states(const T& t, uint64_t q, uint64_t ea, uint64_t eb, uint64_t arr, uint32_t carry,
                     NslBytes x[kNslLanes], uint32_t state[kNslLanes], bool& bad) {
  uint32_t incl[kNslLanes];
  for (uint32_t lane = 0; lane < kNslLanes; ++lane) {
    const uint64_t q0 = q + (uint64_t)kNslLaneBytes * lane;
    x[lane] = nsl_load_bytes(t, q0, ea, eb);
    incl[lane] = nsl_lane_map(x[lane], q0, arr, bad);
  }
  wave_scan_maps(incl);
  for (uint32_t lane = 0; lane < kNslLanes; ++lane)
    state[lane] = nsl_apply(lane ? incl[lane - 1] : kNslIdentity, carry);
  return nsl_apply(incl[kNslLanes - 1], carry);
}

struct EntryCount {
  bool split;
  uint64_t members, bytes;
};

// pass A for the entry at [ea, eb) of the buffer
template <class T>
EntryCount lanes_count(const T& t, uint64_t ea, uint64_t eb) {
  const uint64_t n = eb - ea;
  const EntryCount whole{false, 1, n};
  uint64_t arr = nsl_head(t, n);
  if (arr == kNslFail) return whole;
  arr += ea;
  NslRun run[kNslLanes];
  for (uint32_t lane = 0; lane < kNslLanes; ++lane) run[lane] = NslRun{kNslStart, 0, 0, kNslFail};
  uint32_t carry = kNslStart;
  bool bad = false;
  for (uint64_t q = ea & ~15ull; q < eb; q += kNslStep) {
    NslBytes x[kNslLanes];
    uint32_t state[kNslLanes];
    carry = wave_states(t, q, ea, eb, arr, carry, x, state, bad);
    for (uint32_t lane = 0; lane < kNslLanes; ++lane) {
      run[lane].state = state[lane];
      nsl_lane_replay(x[lane], q + (uint64_t)kNslLaneBytes * lane, arr, run[lane], NslNoEmit{});
    }
  }
  uint64_t members = 0, delta = 0, close = kNslFail;
  for (uint32_t lane = 0; lane < kNslLanes; ++lane) {
    members += run[lane].members;
    delta += run[lane].delta;
    close = run[lane].close < close ? run[lane].close : close;
  }
  if (bad || carry != kNslDone) return whole;
  assert(close != kNslFail && close >= arr && close < eb);
  if (!nsl_tail(t, close - ea + 1, n)) return whole;
  return EntryCount{true, members, delta};
}

// pass B for a split entry: emit(index, body, first) per member, as the kernel's lanes call it
template <class T, class E>
void lanes_emit(const T& t, uint64_t ea, uint64_t eb, E emit) {
  uint64_t arr = nsl_head(t, eb - ea);
  assert(arr != kNslFail);
  arr += ea;
  uint32_t carry = kNslStart;
  uint64_t carry_members = 0, carry_delta = 0;
  bool bad = false;
  for (uint64_t q = ea & ~15ull; q < eb && carry != kNslDone && carry != kNslErr; q += kNslStep) {
    NslBytes x[kNslLanes];
    uint32_t state[kNslLanes];
    carry = wave_states(t, q, ea, eb, arr, carry, x, state, bad);
    uint64_t mem[kNslLanes], del[kNslLanes];
    for (uint32_t lane = 0; lane < kNslLanes; ++lane) {
      NslRun r{state[lane], 0, 0, kNslFail};
      nsl_lane_replay(x[lane], q + (uint64_t)kNslLaneBytes * lane, arr, r, NslNoEmit{});
      mem[lane] = r.members;
      del[lane] = r.delta;
    }
    wave_scan_sums(mem);
    wave_scan_sums(del);
    for (uint32_t lane = 0; lane < kNslLanes; ++lane) {
      NslRun r{state[lane], carry_members + (lane ? mem[lane - 1] : 0), carry_delta + (lane ? del[lane - 1] : 0),
               kNslFail};
      nsl_lane_replay(x[lane], q + (uint64_t)kNslLaneBytes * lane, arr, r, emit);
    }
    carry_members += mem[kNslLanes - 1];
    carry_delta += del[kNslLanes - 1];
  }
}

}  // namespace edv
