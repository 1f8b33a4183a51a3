// small_lanes.h -- the device functions of the single-request kernels (edv_verify_small_kernel,
// edv_resident_kernel): the tree sum of a comb's row points over a wave's lanes, R's decode on the
// lanes (fe_lanes.h) and SHA-512 with the message schedules on the lanes.  Device only.
//
// This is text of edverify.hip, included there at the point it was cut from, inside the
// translation unit's unnamed namespace and after `using namespace edv`; the only other includer is
// tests/native/ed_probe.hip, which runs each function alone against Python integers
// (tests/test_gpu_ed_probe.py) and includes it the same way.  The headers below are already
// included where this one is (they must be: this text sits inside a namespace).
#pragma once
#include "comb.h"
#include "fe_lanes.h"
#include "verify_core.h"

__device__ __forceinline__ void shfl_fe(fe& out, const fe& in, int delta) {
#pragma unroll
  for (int l = 0; l < 10; ++l) out.v[l] = (uint32_t)__shfl_down((int)in.v[l], delta, 64);
}
// Sum of the p3 points of lanes 0..width-1 of this wave (width a power of two
// <= 64; lanes >= rows hold the identity) into lane 0: log2(width) levels of
// p + q (q as cached).
__device__ void lane_tree_sum(ge_p3& P, int lane, int width) {
#pragma unroll 1
  for (int step = 1; step < width; step <<= 1) {
    ge_p3 Q;
    shfl_fe(Q.X, P.X, step);
    shfl_fe(Q.Y, P.Y, step);
    shfl_fe(Q.Z, P.Z, step);
    shfl_fe(Q.T, P.T, step);
    if ((lane & (2 * step - 1)) == 0 && lane < width) {
      ge_cached c;
      ge_p1p1 t;
      ge_p3_to_cached(c, Q);
      ge_add(t, P, c);
      ge_p1p1_to_p3_addlike(P, t);
    }
  }
}
// The point of row `row` of a comb for the signed digit of y (comb_recode'd scalar).
template <int W, class T>
__device__ void comb_row_point(ge_p3& P, const uint32_t y[9], int row, const T& tab) {
  const int e = comb_digit<W>(y, row);
  ge_niels nb;
  tab.load(row, (e < 0 ? -e : e) - 1, nb);
  comb_set_entry(P, nb, e);
}

// libsodium's frombytes of R (ge_frombytes, negate = false) cut in two at a point of its
// exponentiation, so the first ~145 products run beside the hash and the rest beside the key
// comb's tree, with fe_pow22523's chain and the few products before and after it (u, v, v^3,
// u v^7; x, v x^2) spread over wave 2's lanes (fe_lanes.h; ~0.17 us a product on the wave against
// ~0.37 us on lane 0).  Part 1 leaves u = y^2 - 1 (formed as y^2 + 2p - 1 and carried back into
// the dist_* input bounds), v = d y^2 + 1, v^3, u v^7, and t0, t1 and t2 = t1^(2^30) of
// fe_pow22523(u v^7), all distributed (limb k in lane k).
struct RDecodeL {
  uint32_t t0, t1, t2;
  uint32_t du, dv, dv3, duv7;
};
// limb k of a lane-uniform fe in lane k (every lane holds f; no cross-lane moves)
__device__ __forceinline__ uint32_t dist_pick(const fe& f, uint32_t k) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) r = k == (uint32_t)i ? f.v[i] : r;
  return r;
}
__device__ void r_decode_part1_lanes(RDecodeL& d, const uint32_t s[8], uint32_t lane) {
  const uint32_t k = lane & 15;
  const LaneTerms sq = c_lane_sq.t[lane], mu = c_lane_mul.t[lane];
  fe y;
  fe_frombytes(y, s);  // (every lane: the same words)
  const bool row0 = lane < 10;
  const uint32_t yd = k < 10 ? dist_pick(y, k) : 0u;
  const uint32_t y2 = dist_sq(yd, sq, lane);
  // v = d y^2 + 1 (limb 0 of a dist_* output < 2^26: the + 1 stays in bounds)
  const uint32_t dd = k < 10 ? dist_pick(fe_const_d(), k) : 0u;
  d.dv = dist_mul(y2, dd, mu, lane) + (k == 0 ? 1u : 0u);
  // u = y^2 - 1 = y^2 + 2p - 1, carried: limbs of 2p are 2^27 - 38, then 2^26 - 2 / 2^27 - 2
  const uint32_t two_p = k == 0 ? (1u << 27) - 38 : (k & 1) ? (1u << 26) - 2 : (1u << 27) - 2;
  d.du = lane_cols_carry(row0 ? (uint64_t)y2 + two_p - (lane == 0 ? 1u : 0u) : 0ull, lane);
  d.dv3 = dist_mul(dist_sq(d.dv, sq, lane), d.dv, mu, lane);
  d.duv7 = dist_mul(dist_mul(dist_sq(d.dv3, sq, lane), d.dv, mu, lane), d.du, mu, lane);  // u v^7
  const uint32_t zd = d.duv7;
  uint32_t t0 = dist_sq(zd, sq, lane);
  uint32_t t1 = dist_sqn(t0, 2, sq, lane);
  t1 = dist_mul(zd, t1, mu, lane);
  t0 = dist_mul(t0, t1, mu, lane);
  t0 = dist_sq(t0, sq, lane);
  t0 = dist_mul(t1, t0, mu, lane);
  t1 = dist_sqn(t0, 5, sq, lane);
  t0 = dist_mul(t1, t0, mu, lane);
  t1 = dist_sqn(t0, 10, sq, lane);
  t1 = dist_mul(t1, t0, mu, lane);
  uint32_t t2 = dist_sqn(t1, 20, sq, lane);
  t1 = dist_mul(t2, t1, mu, lane);
  t1 = dist_sqn(t1, 10, sq, lane);
  t0 = dist_mul(t1, t0, mu, lane);
  t1 = dist_sqn(t0, 50, sq, lane);
  t1 = dist_mul(t1, t0, mu, lane);
  d.t2 = dist_sqn(t1, 30, sq, lane);
  d.t0 = t0;
  d.t1 = t1;
}
// The rest: x of R with R's sign (false: no square root).  Same value as ge_frombytes.  Every lane
// of the wave calls; x and the result are lane 0's.
__device__ bool r_decode_part2_lanes(fe& x, RDecodeL& d, const uint32_t s[8], uint32_t lane) {
  const LaneTerms sq = c_lane_sq.t[lane], mu = c_lane_mul.t[lane];
  uint32_t t2 = dist_sqn(d.t2, 70, sq, lane);
  uint32_t t1 = dist_mul(t2, d.t1, mu, lane);
  t1 = dist_sqn(t1, 50, sq, lane);
  uint32_t t0 = dist_mul(t1, d.t0, mu, lane);
  t0 = dist_sqn(t0, 2, sq, lane);
  fe vxx, chk;
  // x = u v^3 (u v^7)^((p-5)/8), then v x^2, on the wave; lane 0 takes x, v x^2 and u
  uint32_t xd = dist_mul(dist_mul(dist_mul(t0, d.duv7, mu, lane), d.dv3, mu, lane), d.du, mu, lane);
  const uint32_t vxxd = dist_mul(dist_sq(xd, sq, lane), d.dv, mu, lane);
  fe u;
  dist_to_fe(x, xd);  // class C, in every lane
  dist_to_fe(vxx, vxxd);
  dist_to_fe(u, d.du);
  if (lane != 0) return false;
  fe_sub(chk, vxx, u);
  if (!fe_iszero(chk)) {
    fe_add(chk, vxx, u);
    if (!fe_iszero(chk)) return false;
    fe_mul_chain(x, x, fe_const_sqrtm1());
  }
  if (fe_isnegative(x) != (s[7] >> 31)) {
    fe_neg(x, x);
    fe_carry(x);
  }
  return true;
}

// verify_phase_hash for the single-request kernel: SHA-512(R || A || M) with the blocks' message
// schedules on wave 0's lanes (lane j: block p0 + j of a pass of kHashPass blocks, its 80 words
// into LDS) and only the rounds on lane 0 -- the schedule is ~35 % of a round's instructions, and
// on one lane every instruction is on the critical path.  Every lane of the wave calls; lane 0's
// h and result are verify_phase_hash's.
constexpr int kHashPass = 8;
constexpr int kHashRow = 81;  // u64 per block row (odd: the lanes' rows start in different banks)
__device__ __forceinline__ void sha512_schedule_lds(uint64_t* out, uint64_t w[16]) {
#pragma unroll
  for (int t = 0; t < 16; ++t) out[t] = w[t];
#pragma unroll 1
  for (int r = 16; r < 80; r += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint64_t s0 = xor3_64(rotr64(w15, 1), rotr64(w15, 8), shr64(w15, 7));
      const uint64_t s1 = xor3_64(rotr64(w2, 19), rotr64(w2, 61), shr64(w2, 6));
      w[i] += s0 + w[(i + 9) & 15] + s1;
      out[r + i] = w[i];
    }
  }
}
__device__ __forceinline__ void sha512_rounds_lds(uint64_t st[8], const uint64_t* w) {
  uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
  for (int r = 0; r < 80; r += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint64_t S1 = xor3_64(rotr64(e, 14), rotr64(e, 18), rotr64(e, 41));
      const uint64_t ch = bitop3_64<0xca>(e, f, g);
      const uint64_t t1 = h + S1 + ch + SHA512_K[r + i] + w[r + i];
      const uint64_t S0 = xor3_64(rotr64(a, 28), rotr64(a, 34), rotr64(a, 39));
      const uint64_t mj = bitop3_64<0xe8>(a, b, c);
      h = g;
      g = f;
      f = e;
      e = d + t1;
      d = c;
      c = b;
      b = a;
      a = t1 + S0 + mj;
    }
  }
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
  st[5] += f;
  st[6] += g;
  st[7] += h;
}
__device__ bool verify_phase_hash_lanes(uint32_t hout[8], const uint32_t sig[16], const uint32_t pk[8],
                                        const uint8_t* msg, uint64_t mlen, uint32_t lane, uint64_t* sw) {
  constexpr int NP = 16;
  uint32_t prefix[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    prefix[k] = sig[k];
    prefix[8 + k] = pk[k];
  }
  const uint64_t total = 4 * NP + mlen, nblocks = (total + 16) / 128 + 1, bitlen = total * 8;
  const uint32_t d16 = (uint32_t)((uintptr_t)msg & 15);
  const Chunk16* c16 = (const Chunk16*)(msg - d16);
  const uint64_t nq = (d16 + mlen + 15) / 16;
  uint64_t st[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                    0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
#pragma unroll 1
  for (uint64_t p0 = 0; p0 < nblocks; p0 += kHashPass) {
    const uint64_t b = p0 + lane;
    if (lane < (uint32_t)kHashPass && b < nblocks) {
      uint64_t w[16];
      if (b == 0)
        sha512_block_words<NP, true>(w, 0, prefix, c16, nq, d16, mlen);
      else
        sha512_block_words<NP, false>(w, b, prefix, c16, nq, d16, mlen);
      if (b == nblocks - 1) {
        w[14] = 0;
        w[15] = bitlen;
      }
      sha512_schedule_lds(sw + lane * kHashRow, w);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
      const uint64_t nb = nblocks - p0 < (uint64_t)kHashPass ? nblocks - p0 : (uint64_t)kHashPass;
#pragma unroll 1
      for (uint64_t j = 0; j < nb; ++j) sha512_rounds_lds(st, sw + j * kHashRow);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next pass overwrites sw
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (lane != 0) return false;
  uint32_t digest[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    digest[2 * j] = bswap32((uint32_t)(st[j] >> 32));
    digest[2 * j + 1] = bswap32((uint32_t)st[j]);
  }
  const uint32_t* S = sig + 8;
  const bool ok = sc_is_canonical(S) && !has_small_order(sig) && is_canonical_point(pk) && !has_small_order(pk);
  sc_reduce(hout, digest);
  return ok;
}
