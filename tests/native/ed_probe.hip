// ed_probe.hip -- TEST ONLY: the Ed25519 device arithmetic one primitive at a time, for
// tests/test_gpu_ed_probe.py against Python integers.  Built as libedv_ed_probe.so; the package
// never loads it.  Two kernel shapes: one item per lane (csrc/ed_probe_ops.h, the body shared with
// the CPU twins edv_host_ed_lane / edv_host_ed_hash of csrc/host_check.cpp) and one item per wave
// (csrc/fe_lanes.h and csrc/small_lanes.h: device only, every lane's words copied in and out).
// edprobe_dedup runs the general path's distinct-key dedupe (csrc/key_dedup.h) over one sub-batch
// as the product launches it and returns its arrays (CPU twin: edv_host_ed_dedup).
//
// Host-pointer entry points: each allocates, launches one kernel (block 64), copies back and
// returns the HIP error code (0 = hipSuccess); -1 for an argument the kernel must not see (an
// unknown op, a message outside its buffer, a width that is no power of two).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../indy-plenum_amd/csrc/ed_probe_ops.h"
#include "../../indy-plenum_amd/csrc/fe_lanes.h"

using namespace edv;

namespace {

#include "../../indy-plenum_amd/csrc/small_lanes.h"

constexpr int kBlock = 64;

template <int OP>
__global__ __launch_bounds__(kBlock) void edprobe_lane_kernel(const uint32_t* __restrict__ in, uint64_t n,
                                                             uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  edp::lane_op<OP>(in + (uint64_t)edp::lane_in_words(OP) * i, out + (uint64_t)edp::lane_out_words(OP) * i);
}

// forms 0, 1: one request per lane (edp::hash_op); form 2: one request per wave
// (verify_phase_hash_lanes, sw as SmallShared::sw of edverify.hip)
__global__ __launch_bounds__(kBlock) void edprobe_hash_kernel(int form, const uint32_t* __restrict__ sig,
                                                             const uint32_t* __restrict__ pk, const uint8_t* buf,
                                                             const uint64_t* __restrict__ start,
                                                             const uint64_t* __restrict__ mlen,
                                                             const uint64_t* __restrict__ uoff, Chunk16* units,
                                                             uint64_t n, uint32_t* __restrict__ h_out,
                                                             uint8_t* __restrict__ ok_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h[8];
  const bool ok = edp::hash_op(form, h, sig + 16 * i, pk + 8 * i, buf + start[i], mlen[i], units + uoff[i]);
#pragma unroll
  for (int k = 0; k < 8; ++k) h_out[8 * i + k] = h[k];
  ok_out[i] = ok ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void edprobe_hash_lanes_kernel(const uint32_t* __restrict__ sig,
                                                                   const uint32_t* __restrict__ pk, const uint8_t* buf,
                                                                   const uint64_t* __restrict__ start,
                                                                   const uint64_t* __restrict__ mlen,
                                                                   uint32_t* __restrict__ h_out,
                                                                   uint8_t* __restrict__ ok_out) {
  __shared__ uint64_t sw[kHashPass * kHashRow];
  const uint64_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  uint32_t s[16], a[8], h[8];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = sig[16 * i + k];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = pk[8 * i + k];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = 0;
  const bool ok = verify_phase_hash_lanes(h, s, a, buf + start[i], mlen[i], lane, sw);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) h_out[8 * i + k] = h[k];
    ok_out[i] = ok ? 1 : 0;
  }
}

// the distinct-key dedupe as the product launches it: insert over every request, then assign
__global__ __launch_bounds__(kDedupBlock) void edprobe_dedup_insert_kernel(const uint8_t* __restrict__ pk32, uint64_t n,
                                                                          uint32_t* __restrict__ slots,
                                                                          uint32_t nslots,
                                                                          uint32_t* __restrict__ req_slot,
                                                                          uint32_t* __restrict__ hashes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t pk[8];
  load_key(pk, pk32, i);
  hashes[i] = key_hash(pk);
  dedup_insert(pk32, i, slots, nslots, req_slot);
}
__global__ __launch_bounds__(kDedupBlock) void edprobe_dedup_assign_kernel(uint64_t n, const uint32_t* __restrict__ slots,
                                                                          const uint32_t* __restrict__ req_slot,
                                                                          uint32_t* __restrict__ slot_u,
                                                                          uint32_t* __restrict__ reps,
                                                                          uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dedup_assign(i, slots, req_slot, slot_u, reps, count);
}
// after the assign pass: the split the table and ladder kernels take
__global__ void edprobe_split_kernel(const uint32_t* __restrict__ count, uint64_t n, int* __restrict__ split) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *split = split_of(*count, n);
}

// ---- one item per wave.  Words per item in / out:
enum : int { kDistSq, kDistMul, kDistSqn, kColsCarry, kDistRound, kRDecode, kTreeSum, kWaveOps };
constexpr int wave_in_words(int op) {
  return op == kDistSq || op == kDistSqn ? 64      // f of every lane
         : op == kDistMul ? 128                   // f, g of every lane
         : op == kColsCarry ? 128                 // the low, then the high words of every lane's p
         : op == kDistRound ? 640                 // an fe (10 limbs) in every lane; lane 0's is read
         : op == kRDecode ? 8                     // R's encoding, the same words in every lane
         : op == kTreeSum ? 2560 : -1;            // a p3 point (40 words) in every lane
}
constexpr int wave_out_words(int op) {
  return op == kDistSq || op == kDistSqn || op == kDistMul || op == kColsCarry ? 64  // every lane's result
         : op == kDistRound ? 64 + 640  // every lane's distributed word, then every lane's fe of dist_to_fe
         : op == kRDecode ? 9           // lane 0's flag, fe_tobytes(x)
         : op == kTreeSum ? 40 : -1;    // lane 0's point
}

template <int OP>
__global__ __launch_bounds__(kBlock) void edprobe_wave_kernel(const uint32_t* __restrict__ in_all, uint32_t aux,
                                                             uint32_t* __restrict__ out_all) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* in = in_all + (uint64_t)wave_in_words(OP) * blockIdx.x;
  uint32_t* out = out_all + (uint64_t)wave_out_words(OP) * blockIdx.x;
  if constexpr (OP == kDistSq) {
    out[lane] = dist_sq(in[lane], c_lane_sq.t[lane], lane);
  } else if constexpr (OP == kDistSqn) {
    out[lane] = dist_sqn(in[lane], (int)aux, c_lane_sq.t[lane], lane);
  } else if constexpr (OP == kDistMul) {
    out[lane] = dist_mul(in[lane], in[64 + lane], c_lane_mul.t[lane], lane);
  } else if constexpr (OP == kColsCarry) {
    out[lane] = lane_cols_carry(((uint64_t)in[64 + lane] << 32) | in[lane], lane);
  } else if constexpr (OP == kDistRound) {
    fe f, g;
    load_fe(f, in + 10 * lane);
    const uint32_t d = dist_from_lane0(f, lane);
    dist_to_fe(g, d);
    out[lane] = d;
    store_fe(out + 64 + 10 * lane, g);
  } else if constexpr (OP == kRDecode) {
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = in[k];
    RDecodeL d;
    r_decode_part1_lanes(d, s, lane);
    fe x;
    const bool ok = r_decode_part2_lanes(x, d, s, lane);
    if (lane == 0) {
      uint32_t w[8];
      fe_tobytes(w, x);
      out[0] = ok ? 1u : 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) out[1 + k] = w[k];
    }
  } else {
    static_assert(OP == kTreeSum, "every op has a body");
    ge_p3 P;
    edp::load_p3(P, in + 40 * lane);
    lane_tree_sum(P, (int)lane, (int)aux);
    if (lane == 0) edp::store_p3(out, P);
  }
}

struct Bufs {
  std::vector<void*> p;
  ~Bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipSuccess) p.push_back(*out);
    return e;
  }
  // a device copy of bytes of host memory
  hipError_t copy_in(void** out, const void* src, size_t bytes) {
    hipError_t e = alloc(out, bytes);
    return e != hipSuccess || bytes == 0 ? e : hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice);
  }
};

#define PROBE_TRY(expr)              \
  do {                               \
    hipError_t e_ = (expr);          \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

template <int OP>
void launch_lane(const uint32_t* d_in, uint64_t n, uint32_t* d_out) {
  hipLaunchKernelGGL(edprobe_lane_kernel<OP>, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, d_in, n,
                     d_out);
}
template <int OP>
void launch_wave(const uint32_t* d_in, uint32_t aux, uint64_t n, uint32_t* d_out) {
  hipLaunchKernelGGL(edprobe_wave_kernel<OP>, dim3((uint32_t)n), dim3(kBlock), 0, 0, d_in, aux, d_out);
}

}  // namespace

extern "C" {

// the base comb's window in this build (kBaseW)
int edprobe_base_w(void) { return edv::kBaseW; }
// io[0], io[1] = the words of one item of lane op `op` in and out; -1 for an unknown op
int edprobe_lane_io(int op, int io[2]) {
  if (op < 0 || op >= edp::kLaneOps) return -1;
  io[0] = edp::lane_in_words(op);
  io[1] = edp::lane_out_words(op);
  return 0;
}
// the op of ed_probe_ops.h over n items, one per lane
int edprobe_lane(int op, const uint32_t* in, uint64_t n, uint32_t* out) {
  if (op < 0 || op >= edp::kLaneOps || n > 0x7fffffffull) return -1;
  if (op == edp::kFeSqn)  // the squaring count is the item's: keep the kernel's loop short
    for (uint64_t i = 0; i < n; ++i)
      if (in[11 * i + 10] < 1 || in[11 * i + 10] > 300) return -1;
  if (n == 0) return 0;
  const size_t in_b = 4 * (size_t)edp::lane_in_words(op) * n, out_b = 4 * (size_t)edp::lane_out_words(op) * n;
  Bufs bufs;
  void *d_in, *d_out;
  PROBE_TRY(bufs.copy_in(&d_in, in, in_b));
  PROBE_TRY(bufs.alloc(&d_out, out_b));
  switch (op) {
#define EDV_CASE(OP) \
  case OP: launch_lane<OP>((const uint32_t*)d_in, n, (uint32_t*)d_out); break;
    EDV_ED_LANE_OPS(EDV_CASE)
#undef EDV_CASE
  }
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  return 0;
}

// h = SHA-512(R || A || M) mod L and the four prechecks of n requests: form 0 verify_phase_hash,
// 1 pack_lane_units + verify_phase_hash_units, 2 verify_phase_hash_lanes (a wave per request).
// Request i's message is buf[start[i] .. start[i] + mlen[i]); the device copy of buf starts on a
// 16-byte boundary and is padded to whole 16-byte chunks, so start[i] mod 16 is the message's
// alignment and the bytes around it inside its chunks are the caller's.
int edprobe_hash(int form, const uint8_t* sig64, const uint8_t* pk32, const uint8_t* buf, uint64_t buf_len,
                 const uint64_t* start, const uint64_t* mlen, uint64_t n, uint32_t* h_out, uint8_t* ok_out) {
  if (form < 0 || form > 2 || n > 0x7fffffffull) return -1;
  std::vector<uint64_t> uoff(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (start[i] > buf_len || mlen[i] > buf_len - start[i]) return -1;
    uoff[i + 1] = uoff[i] + (form == 1 ? sha512_units64(mlen[i]) : 0);
  }
  if (n == 0) return 0;
  Bufs bufs;
  void *d_sig, *d_pk, *d_buf, *d_start, *d_mlen, *d_uoff, *d_units, *d_h, *d_ok;
  PROBE_TRY(bufs.copy_in(&d_sig, sig64, 64 * n));
  PROBE_TRY(bufs.copy_in(&d_pk, pk32, 32 * n));
  PROBE_TRY(bufs.alloc(&d_buf, (buf_len + 15) / 16 * 16 + 16));
  PROBE_TRY(hipMemset(d_buf, 0, (buf_len + 15) / 16 * 16 + 16));
  if (buf_len) PROBE_TRY(hipMemcpy(d_buf, buf, buf_len, hipMemcpyHostToDevice));
  PROBE_TRY(bufs.copy_in(&d_start, start, 8 * n));
  PROBE_TRY(bufs.copy_in(&d_mlen, mlen, 8 * n));
  PROBE_TRY(bufs.copy_in(&d_uoff, uoff.data(), 8 * n));
  PROBE_TRY(bufs.alloc(&d_units, 16 * uoff[n]));
  PROBE_TRY(bufs.alloc(&d_h, 32 * n));
  PROBE_TRY(bufs.alloc(&d_ok, n));
  if (form == 2)
    hipLaunchKernelGGL(edprobe_hash_lanes_kernel, dim3((uint32_t)n), dim3(kBlock), 0, 0, (const uint32_t*)d_sig,
                       (const uint32_t*)d_pk, (const uint8_t*)d_buf, (const uint64_t*)d_start, (const uint64_t*)d_mlen,
                       (uint32_t*)d_h, (uint8_t*)d_ok);
  else
    hipLaunchKernelGGL(edprobe_hash_kernel, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, form,
                       (const uint32_t*)d_sig, (const uint32_t*)d_pk, (const uint8_t*)d_buf, (const uint64_t*)d_start,
                       (const uint64_t*)d_mlen, (const uint64_t*)d_uoff, (Chunk16*)d_units, n, (uint32_t*)d_h,
                       (uint8_t*)d_ok);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(h_out, d_h, 32 * n, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(ok_out, d_ok, n, hipMemcpyDeviceToHost));
  return 0;
}

// The distinct-key dedupe of one sub-batch of n requests (keys pk32, 32 bytes each) over nslots
// slots, with the product's kernels' bodies and block size (csrc/key_dedup.h): slots cleared to
// 0xff, the insert pass, the assign pass.  Out: slots[nslots], req_slot[n], slot_u[nslots] (0xff
// where no representative wrote), reps[n] (0xff past the count), the distinct count, key_hash of
// every request's key and split_of(count, n).  -1 without a launch for n == 0, nslots < n or
// n > 4096 (edp::dedup_args_ok).
int edprobe_dedup(const uint8_t* pk32, uint64_t n, uint64_t nslots, uint32_t* slots, uint32_t* req_slot,
                  uint32_t* slot_u, uint32_t* reps, uint32_t* count, uint32_t* hashes, int* split) {
  if (!edp::dedup_args_ok(n, nslots)) return -1;
  Bufs bufs;
  void *d_pk, *d_slots, *d_req, *d_su, *d_reps, *d_count, *d_hash, *d_split;
  PROBE_TRY(bufs.copy_in(&d_pk, pk32, 32 * n));
  PROBE_TRY(bufs.alloc(&d_slots, 4 * nslots));
  PROBE_TRY(bufs.alloc(&d_req, 4 * n));
  PROBE_TRY(bufs.alloc(&d_su, 4 * nslots));
  PROBE_TRY(bufs.alloc(&d_reps, 4 * n));
  PROBE_TRY(bufs.alloc(&d_count, 4));
  PROBE_TRY(bufs.alloc(&d_hash, 4 * n));
  PROBE_TRY(bufs.alloc(&d_split, sizeof(int)));
  PROBE_TRY(hipMemset(d_slots, 0xff, 4 * nslots));
  PROBE_TRY(hipMemset(d_req, 0xff, 4 * n));
  PROBE_TRY(hipMemset(d_su, 0xff, 4 * nslots));
  PROBE_TRY(hipMemset(d_reps, 0xff, 4 * n));
  PROBE_TRY(hipMemset(d_count, 0, 4));
  PROBE_TRY(hipMemset(d_split, 0, sizeof(int)));
  const dim3 grid((uint32_t)((n + kDedupBlock - 1) / kDedupBlock)), block(kDedupBlock);
  hipLaunchKernelGGL(edprobe_dedup_insert_kernel, grid, block, 0, 0, (const uint8_t*)d_pk, n, (uint32_t*)d_slots,
                     (uint32_t)nslots, (uint32_t*)d_req, (uint32_t*)d_hash);
  PROBE_TRY(hipGetLastError());
  hipLaunchKernelGGL(edprobe_dedup_assign_kernel, grid, block, 0, 0, n, (const uint32_t*)d_slots,
                     (const uint32_t*)d_req, (uint32_t*)d_su, (uint32_t*)d_reps, (uint32_t*)d_count);
  PROBE_TRY(hipGetLastError());
  hipLaunchKernelGGL(edprobe_split_kernel, dim3(1), dim3(kBlock), 0, 0, (const uint32_t*)d_count, n, (int*)d_split);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(slots, d_slots, 4 * nslots, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(req_slot, d_req, 4 * n, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(slot_u, d_su, 4 * nslots, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(reps, d_reps, 4 * n, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(count, d_count, 4, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(hashes, d_hash, 4 * n, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(split, d_split, sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// io[0], io[1] = the words of one item of wave op `op` in and out; -1 for an unknown op
int edprobe_wave_io(int op, int io[2]) {
  if (op < 0 || op >= kWaveOps) return -1;
  io[0] = wave_in_words(op);
  io[1] = wave_out_words(op);
  return 0;
}
// op: 0 dist_sq, 1 dist_mul, 2 dist_sqn (aux squarings), 3 lane_cols_carry, 4 dist_from_lane0 ->
// dist_to_fe, 5 r_decode_part1_lanes + r_decode_part2_lanes, 6 lane_tree_sum (width aux: 2..64, a
// power of two); n items, one per wave
int edprobe_wave(int op, const uint32_t* in, uint32_t aux, uint64_t n, uint32_t* out) {
  if (op < 0 || op >= kWaveOps || n > 0x7fffffffull) return -1;
  if (op == kTreeSum && (aux < 2 || aux > 64 || (aux & (aux - 1)))) return -1;
  if (op == kDistSqn && aux > 1000) return -1;
  if (n == 0) return 0;
  const size_t in_b = 4 * (size_t)wave_in_words(op) * n, out_b = 4 * (size_t)wave_out_words(op) * n;
  Bufs bufs;
  void *d_in, *d_out;
  PROBE_TRY(bufs.copy_in(&d_in, in, in_b));
  PROBE_TRY(bufs.alloc(&d_out, out_b));
  switch (op) {
#define EDV_CASE(OP) \
  case OP: launch_wave<OP>((const uint32_t*)d_in, aux, n, (uint32_t*)d_out); break;
    EDV_CASE(kDistSq) EDV_CASE(kDistMul) EDV_CASE(kDistSqn) EDV_CASE(kColsCarry) EDV_CASE(kDistRound)
    EDV_CASE(kRDecode) EDV_CASE(kTreeSum)
#undef EDV_CASE
  }
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
