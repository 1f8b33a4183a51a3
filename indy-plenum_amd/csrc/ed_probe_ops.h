// ed_probe_ops.h -- TEST ONLY: one Ed25519 primitive per call on raw words, the shared body of
// tests/native/ed_probe.hip (one item per lane on the device) and of its CPU twins
// edv_host_ed_* (csrc/host_check.cpp, with the EDV_BOUND_CHECK assertions), so both run the same
// calls on the same words and a difference between them is the device's.  The product never
// includes this file.
//
// An item of op OP is lane_in_words(OP) input words and lane_out_words(OP) output words; field
// elements are 10 raw limbs (not reduced: the tests pass limbs at the class bounds), points are
// X, Y, Z, T (40 words), niels entries y+x, y-x, 2dxy (30 words), byte strings 8 LE words, a
// signature slot (sig_slot.h) its 24 LE words.
#pragma once
#include "key_dedup.h"
#include "sig_slot.h"
#include "verify_core.h"

namespace edv {
namespace edp {

enum : int {
  kFeMul, kFeSq, kFeSqn, kFeAdd, kFeSub, kFeSub4, kFeNeg, kFeCarry, kFeTobytes, kFeFrombytes, kFeInvert,
  kFePow22523, kFeIszero, kFeIsnegative, kFeCmov,
  kScReduce, kScIsCanonical, kScMuladd, kRecode16, kComb10, kComb14, kComb16, kCombBase,
  kGeFrombytes, kHasSmallOrder, kIsCanonicalPoint, kGeAdd, kGeSub, kGeMadd, kGeMsub, kGeAddSigned, kP2Dbl, kP3Dbl,
  kCombSetEntry, kGeTobytes, kSigSlot,
  kLaneOps
};
constexpr int kCombOutWords = 27;  // the row count, then up to 26 digits (W = 10), zero past the rows

EDV_HD constexpr int lane_in_words(int op) {
  switch (op) {
    case kFeMul: case kFeAdd: case kFeSub: case kFeSub4: return 20;
    case kFeSqn: return 11;   // f, n
    case kFeCmov: return 21;  // f, h, b
    case kFeFrombytes: case kScIsCanonical: case kRecode16: case kComb10: case kComb14: case kComb16:
    case kCombBase: case kHasSmallOrder: case kIsCanonicalPoint: return 8;
    case kScReduce: return 16;
    case kScMuladd: return 24;     // a, b, c
    case kSigSlot: return 24;      // an EDV_SIG_SLOT96 slot
    case kGeFrombytes: return 9;   // s, negate
    case kGeAdd: case kGeSub: return 80;  // p (p3), q (p3: made cached as the callers do)
    case kGeMadd: case kGeMsub: return 70;  // p (p3), q (niels)
    case kGeAddSigned: return 81;  // p, q, neg
    case kP2Dbl: case kP3Dbl: return 40;
    case kCombSetEntry: return 31;  // niels, e
    case kGeTobytes: return 30;     // X, Y, Z
    default: return op >= 0 && op < kLaneOps ? 10 : -1;
  }
}
EDV_HD constexpr int lane_out_words(int op) {
  switch (op) {
    case kFeTobytes: case kScReduce: case kScMuladd: case kGeTobytes: return 8;
    case kFeIszero: case kFeIsnegative: case kScIsCanonical: case kHasSmallOrder: case kIsCanonicalPoint: return 1;
    case kRecode16: return 64;
    case kSigSlot: return 16;  // R || S
    case kComb10: case kComb14: case kComb16: case kCombBase: return kCombOutWords;
    case kGeFrombytes: return 41;  // ok, then the point
    case kGeAdd: case kGeSub: case kGeMadd: case kGeMsub: case kGeAddSigned: case kP2Dbl: case kP3Dbl:
    case kCombSetEntry: return 40;
    default: return op >= 0 && op < kLaneOps ? 10 : -1;
  }
}

EDV_HD void load_p3(ge_p3& P, const uint32_t* p) {
  load_fe(P.X, p);
  load_fe(P.Y, p + 10);
  load_fe(P.Z, p + 20);
  load_fe(P.T, p + 30);
}
EDV_HD void store_p3(uint32_t* p, const ge_p3& P) {
  store_fe(p, P.X);
  store_fe(p + 10, P.Y);
  store_fe(p + 20, P.Z);
  store_fe(p + 30, P.T);
}
EDV_HD void load_niels(ge_niels& n, const uint32_t* p) {
  load_fe(n.ypx, p);
  load_fe(n.ymx, p + 10);
  load_fe(n.xy2d, p + 20);
}
template <int W>
EDV_HD void comb_digits(uint32_t* out, const uint32_t x[8]) {
  static_assert(Window<W>::kRows < kCombOutWords, "digits fit the item");
  uint32_t y[9];
  comb_recode<W>(y, x);
  out[0] = (uint32_t)Window<W>::kRows;
  for (int r = 0; r + 1 < kCombOutWords; ++r) out[1 + r] = r < Window<W>::kRows ? (uint32_t)comb_digit<W>(y, r) : 0u;
}

template <int OP>
EDV_HD void lane_op(const uint32_t* in, uint32_t* out) {
  static_assert(OP >= 0 && OP < kLaneOps, "a lane op");
  uint32_t w[24];  // the byte-string and scalar operands, out of the caller's memory
  for (int k = 0; k < 24; ++k) w[k] = k < lane_in_words(OP) ? in[k] : 0u;
  if constexpr (OP <= kFeCmov) {
    fe f, g, h;
    load_fe(f, w);
    load_fe(g, w + 10);
    uint32_t o[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fe_0(h);
    if constexpr (OP == kFeMul) fe_mul_chain(h, f, g);
    if constexpr (OP == kFeSq) fe_sq_chain(h, f);
    if constexpr (OP == kFeSqn) fe_sqn(h, f, (int)w[10]);
    if constexpr (OP == kFeAdd) fe_add(h, f, g);
    if constexpr (OP == kFeSub) fe_sub(h, f, g);
    if constexpr (OP == kFeSub4) fe_sub4(h, f, g);
    if constexpr (OP == kFeNeg) fe_neg(h, f);
    if constexpr (OP == kFeCarry) {
      h = f;
      fe_carry(h);
    }
    if constexpr (OP == kFeInvert) fe_invert(h, f);
    if constexpr (OP == kFePow22523) fe_pow22523(h, f);
    if constexpr (OP == kFeCmov) {
      h = g;
      fe_cmov(h, f, (w[20] & 1u) != 0);
    }
    store_fe(o, h);
    if constexpr (OP == kFeTobytes) fe_tobytes(o, f);
    if constexpr (OP == kFeFrombytes) {
      fe_frombytes(h, w);
      store_fe(o, h);
    }
    if constexpr (OP == kFeIszero) o[0] = fe_iszero(f) ? 1u : 0u;
    if constexpr (OP == kFeIsnegative) o[0] = fe_isnegative(f);
    for (int k = 0; k < lane_out_words(OP); ++k) out[k] = o[k];
  } else if constexpr (OP == kScReduce) {
    uint32_t o[8];
    sc_reduce(o, w);
    for (int k = 0; k < 8; ++k) out[k] = o[k];
  } else if constexpr (OP == kScIsCanonical) {
    out[0] = sc_is_canonical(w) ? 1u : 0u;
  } else if constexpr (OP == kScMuladd) {
    uint32_t o[8];
    sc_muladd(o, w, w + 8, w + 16);
    for (int k = 0; k < 8; ++k) out[k] = o[k];
  } else if constexpr (OP == kRecode16) {
    uint32_t y[8];
    sc_recode16(y, w);
    for (int i = 0; i < 64; ++i) out[i] = (uint32_t)recode_digit(y, i);
  } else if constexpr (OP == kComb10) {
    comb_digits<10>(out, w);
  } else if constexpr (OP == kComb14) {
    comb_digits<14>(out, w);
  } else if constexpr (OP == kComb16) {
    comb_digits<16>(out, w);
  } else if constexpr (OP == kCombBase) {
    comb_digits<kBaseW>(out, w);
  } else if constexpr (OP == kGeFrombytes) {
    ge_p3 P;
    out[0] = ge_frombytes(P, w, (w[8] & 1u) != 0) ? 1u : 0u;
    store_p3(out + 1, P);
  } else if constexpr (OP == kHasSmallOrder) {
    out[0] = has_small_order(w) ? 1u : 0u;
  } else if constexpr (OP == kIsCanonicalPoint) {
    out[0] = is_canonical_point(w) ? 1u : 0u;
  } else if constexpr (OP == kGeTobytes) {
    ge_p2 q;
    load_fe(q.X, in);
    load_fe(q.Y, in + 10);
    load_fe(q.Z, in + 20);
    uint32_t o[8];
    ge_tobytes(o, q);
    for (int k = 0; k < 8; ++k) out[k] = o[k];
  } else if constexpr (OP == kSigSlot) {
    uint32_t o[16];
    sig_slot_decode(o, w);
    for (int k = 0; k < 16; ++k) out[k] = o[k];
  } else if constexpr (OP == kCombSetEntry) {
    ge_niels nb;
    load_niels(nb, in);
    ge_p3 R;
    comb_set_entry(R, nb, (int)in[30]);
    store_p3(out, R);
  } else {
    ge_p3 P, Q, R;
    load_p3(P, in);
    ge_p1p1 t;
    if constexpr (OP == kGeAdd || OP == kGeSub || OP == kGeAddSigned) {
      load_p3(Q, in + 40);
      ge_cached c;
      ge_p3_to_cached(c, Q);
      if constexpr (OP == kGeAdd) {
        ge_add(t, P, c);
        ge_p1p1_to_p3_addlike(R, t);
      } else if constexpr (OP == kGeSub) {
        ge_sub(t, P, c);
        ge_p1p1_to_p3_sublike(R, t);
      } else {
        ge_add_signed(R, P, c, (in[80] & 1u) != 0);
      }
    } else if constexpr (OP == kGeMadd || OP == kGeMsub) {
      ge_niels nb;
      load_niels(nb, in + 40);
      if constexpr (OP == kGeMadd) {
        ge_madd(t, P, nb);
        ge_p1p1_to_p3_addlike(R, t);
      } else {
        ge_msub(t, P, nb);
        ge_p1p1_to_p3_sublike(R, t);
      }
    } else if constexpr (OP == kP2Dbl) {
      ge_p2 q;
      ge_p3_to_p2(q, P);
      ge_p2_dbl(t, q);
      ge_dbl_to_p3(R, t);
    } else {
      static_assert(OP == kP3Dbl, "every op has a body");
      ge_p3_dbl(t, P);
      ge_dbl_to_p3(R, t);
    }
    store_p3(out, R);
  }
}

// The hash phase of one request in the two one-lane forms: form 0 verify_phase_hash, form 1
// pack_lane_units (into units, sha512_units64(mlen) chunks at stride 1) then
// verify_phase_hash_units.
EDV_HD bool hash_op(int form, uint32_t h[8], const uint32_t sig[16], const uint32_t pk[8], const uint8_t* msg,
                    uint64_t mlen, Chunk16* units) {
  if (form == 0) return verify_phase_hash(h, sig, pk, msg, mlen);
  pack_lane_units(units, 1, msg, mlen);
  return verify_phase_hash_units(h, sig, pk, units, 1, mlen);
}

// The distinct-key dedupe of one sub-batch (key_dedup.h: dedup_insert for every request, then
// dedup_assign for every request, as edv_dedup_insert_kernel and edv_dedup_assign_kernel run
// them).  Both entry points refuse, before they run anything, a batch whose table could fill up
// or whose probe walk could be long: no request, fewer slots than requests, more than 4096.
constexpr uint64_t kDedupMaxN = 4096;
inline bool dedup_args_ok(uint64_t n, uint64_t nslots) {
  return n >= 1 && n <= kDedupMaxN && nslots >= n && nslots <= 2 * kDedupMaxN;
}

// X(op) for every lane op, for the switches of the two builds
#define EDV_ED_LANE_OPS(X)                                                                                         \
  X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
  X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35)
static_assert(kLaneOps == 36, "EDV_ED_LANE_OPS lists every op");

}  // namespace edp
}  // namespace edv
