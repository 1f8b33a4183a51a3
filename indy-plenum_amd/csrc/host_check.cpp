// host_check.cpp -- TEST INFRASTRUCTURE: the kernel arithmetic (verify_core.h
// and friends) compiled for the host CPU with EDV_BOUND_CHECK limb-bound
// assertions, so tests/ can check the exact device code paths against the
// oracle without a GPU.  The product (libplenum_edverify.so) never links this.
#include <string.h>

#include <vector>

#include "batch_encode.h"
#include "bn254.h"
#include "comb.h"
#include "sha256.h"
#include "verify_core.h"

using namespace edv;

namespace {
struct HostTableA {
  ge_cached e[9];  // slot 8: the identity
  void store(int j, const ge_cached& c) { e[j] = c; }
  void load(int j, ge_cached& c) const { c = e[j >= 0 ? j : 8]; }
};
template <int K>
struct HostTableSplit {
  HostTableA t[K];
  void store(int s, int j, const ge_cached& c) const { const_cast<HostTableA&>(t[s]).store(j, c); }
  void load(int s, int j, ge_cached& c) const { t[s].load(j, c); }
};
// A comb table in host memory (comb.h layout).
template <int W>
struct HostComb {
  const uint32_t* tab;
  void load(int row, int j, ge_niels& n) const {
    const uint32_t* p = j >= 0 ? tab + ((size_t)row * Window<W>::kEntries + j) * kEntryWords : kNielsIdentityHost;
    memcpy(n.ypx.v, p, 40);
    memcpy(n.ymx.v, p + 10, 40);
    memcpy(n.xy2d.v, p + 20, 40);
  }
};

std::vector<uint32_t> g_btab;  // W = 8 comb of B, built by the device code on first use

template <int W>
void build_table(std::vector<uint32_t>& tab, const ge_p3& P) {
  constexpr int rows = Window<W>::kRows, E = Window<W>::kEntries;
  std::vector<uint32_t> rw(rows * 40), pre(32 * 10);
  tab.assign((size_t)rows * E * kEntryWords, 0);
  comb_rows<W>(rw.data(), P);
  // strided lanes of up to 32 entries, as edv_comb_fill_kernel fills them
  const int CH = E < 32 ? E : 32, NCH = E / CH;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < NCH; ++c)
      comb_fill_strided(&tab[(size_t)r * E * kEntryWords], pre.data(), 10, &rw[r * 40], c, NCH, CH);
}

const uint32_t* base_comb() {
  if (g_btab.empty()) {
    uint32_t b[8];
    for (int k = 0; k < 8; ++k) b[k] = 0x66666666u;
    b[0] = 0x66666658u;
    ge_p3 B;
    ge_frombytes(B, b, false);
    build_table<kBaseW>(g_btab, B);
  }
  return g_btab.data();
}
}  // namespace

extern "C" {

int edv_host_verify(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* msg, uint64_t mlen) {
  uint32_t sig[16], pk[8];
  memcpy(sig, sig64, 64);
  memcpy(pk, pk32, 32);
  HostTableA ta;
  const HostComb<kBaseW> cb{base_comb()};
  return verify_one(sig, pk, msg, mlen, ta, cb) ? 0 : -1;
}

// The general path's split-table ladder (K tables of 2^(256t/K)(-A)), as
// edv_table_kernel / edv_dsm_kernel run it for keys shared by >= 4 requests.
int edv_host_verify_split(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* msg, uint64_t mlen, int k) {
  uint32_t sig[16], pk[8], h[8];
  memcpy(sig, sig64, 64);
  memcpy(pk, pk32, 32);
  const HostComb<kBaseW> cb{base_comb()};
  bool ok = verify_phase_hash(h, sig, pk, msg, mlen);
  ge_p3 Q;
  if (k == 8) {
    HostTableSplit<8> tas;
    ok = verify_phase_table_split<8>(pk, tas) && ok;
    verify_phase_dsm_split_point<8>(Q, h, sig + 8, tas, cb);
  } else if (k == 4) {
    HostTableSplit<4> tas;
    ok = verify_phase_table_split<4>(pk, tas) && ok;
    verify_phase_dsm_split_point<4>(Q, h, sig + 8, tas, cb);
  } else if (k == 2) {
    HostTableSplit<2> tas;
    ok = verify_phase_table_split<2>(pk, tas) && ok;
    verify_phase_dsm_split_point<2>(Q, h, sig + 8, tas, cb);
  } else {
    HostTableSplit<1> tas;
    ok = verify_phase_table_split<1>(pk, tas) && ok;
    verify_phase_dsm_split_point<1>(Q, h, sig + 8, tas, cb);
  }
  return encode_equals(Q, sig) && ok ? 0 : -1;
}

void edv_host_sha512_prefixed(uint8_t out[64], const uint8_t prefix64[64], const uint8_t* msg, uint64_t mlen) {
  uint32_t pre[16], dig[16];
  memcpy(pre, prefix64, 64);
  sha512_prefixed<16>(dig, pre, msg, mlen);
  memcpy(out, dig, 64);
}

// The packed unit layout: M packed into units at `stride` (a lane of a
// lane-interleaved group), then hashed from them; also hands the units back.
void edv_host_sha512_units(uint8_t out[64], const uint8_t prefix64[64], const uint8_t* msg, uint64_t mlen,
                           uint64_t stride, uint8_t* units_out) {
  uint32_t pre[16], dig[16];
  memcpy(pre, prefix64, 64);
  const uint64_t nu = sha512_units64(mlen);
  std::vector<Chunk16> u(nu * stride, Chunk16{0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu});
  pack_lane_units(u.data(), stride, msg, mlen);
  sha512_prefixed_units(dig, pre, u.data(), stride, mlen);
  memcpy(out, dig, 64);
  if (units_out)
    for (uint64_t p = 0; p < nu; ++p) memcpy(units_out + 16 * p, &u[p * stride], 16);
}
uint64_t edv_host_sha512_units_count(uint64_t mlen) { return sha512_units64(mlen); }

void edv_host_sha256(uint8_t out[32], const uint8_t* msg, uint64_t mlen) {
  uint32_t d[8];
  sha256_msg(d, msg, mlen);
  memcpy(out, d, 32);
}

void edv_host_sc_reduce(uint8_t out[32], const uint8_t in[64]) {
  uint32_t i[16], o[8];
  memcpy(i, in, 64);
  sc_reduce(o, i);
  memcpy(out, o, 32);
}

int edv_host_sc_is_canonical(const uint8_t s[32]) {
  uint32_t w[8];
  memcpy(w, s, 32);
  return sc_is_canonical(w);
}

// out = canonical bytes of (a * b) for field elements given as 32-byte LE
// integers < 2^255 (exercises fe_frombytes, fe_mul, fe_sq, fe_tobytes).
// mode: bit 0 square
static void fe_mul_mode(fe& fo, const fe& fa, const fe& fb, int mode) {
  (mode & 1) ? fe_sq(fo, fa) : fe_mul(fo, fa, fb);
  EDV_ASSERT(EDV_IS_C(fo));
}
void edv_host_fe_mul(uint8_t out[32], const uint8_t a[32], const uint8_t b[32], int mode) {
  uint32_t wa[8], wb[8], wo[8];
  memcpy(wa, a, 32);
  memcpy(wb, b, 32);
  fe fa, fb, fo;
  fe_frombytes(fa, wa);
  fe_frombytes(fb, wb);
  fe_mul_mode(fo, fa, fb, mode);
  fe_tobytes(wo, fo);
  memcpy(out, wo, 32);
}
// The same on raw limbs (a in W, b in L; a in L when squaring): out = the product's limbs (class C).
void edv_host_fe_mul_limbs(uint32_t out[10], const uint32_t a[10], const uint32_t b[10], int mode) {
  fe fa, fb, fo;
  memcpy(fa.v, a, 40);
  memcpy(fb.v, b, 40);
  fe_mul_mode(fo, fa, fb, mode);
  memcpy(out, fo.v, 40);
}

void edv_host_fe_invert(uint8_t out[32], const uint8_t a[32]) {
  uint32_t wa[8], wo[8];
  memcpy(wa, a, 32);
  fe fa, fo;
  fe_frombytes(fa, wa);
  fe_invert(fo, fa);
  fe_tobytes(wo, fo);
  memcpy(out, wo, 32);
}

// Decode (negate = 0) and re-encode a point; -1 if not on the curve.
int edv_host_point_roundtrip(uint8_t out[32], const uint8_t in[32]) {
  uint32_t w[8], o[8];
  memcpy(w, in, 32);
  ge_p3 P;
  if (!ge_frombytes(P, w, false)) return -1;
  ge_p2 p2;
  ge_p3_to_p2(p2, P);
  ge_tobytes(o, p2);
  memcpy(out, o, 32);
  return 0;
}

int edv_host_has_small_order(const uint8_t s[32]) {
  uint32_t w[8];
  memcpy(w, s, 32);
  return has_small_order(w);
}

int edv_host_is_canonical_point(const uint8_t s[32]) {
  uint32_t w[8];
  memcpy(w, s, 32);
  return is_canonical_point(w);
}

}  // extern "C"

// The key-table (comb) path on the CPU: build the W-window table of -A and
// the W = 8 table of B with the device code, then [h](-A) + [S]B by the comb
// (comb_mul_add, the kernel's code).  Result point and the combined prechecks.
// The key's table, kept from call to call while the key stays the same (per thread and window).
template <int W>
static const std::vector<uint32_t>& key_table(const uint32_t pk[8], const ge_p3& A) {
  thread_local std::vector<uint32_t> tab;
  thread_local uint32_t have[8];
  if (tab.empty() || memcmp(have, pk, 32) != 0) {
    build_table<W>(tab, A);
    memcpy(have, pk, 32);
  }
  return tab;
}

template <int W>
static bool comb_point(ge_p3& Q, const uint32_t sig[16], const uint32_t pk[8], const uint8_t* msg, uint64_t mlen) {
  uint32_t h[8];
  bool ok = verify_phase_hash(h, sig, pk, msg, mlen);
  ge_p3 A;
  ok = ge_frombytes(A, pk, true) && is_canonical_point(pk) && !has_small_order(pk) && ok;
  const std::vector<uint32_t>& atab = key_table<W>(pk, A);
  comb_mul_set<W>(Q, h, HostComb<W>{atab.data()});
  comb_mul_add<kBaseW>(Q, sig + 8, HostComb<kBaseW>{base_comb()});
  return ok;
}

static bool comb_point_w(int w, ge_p3& Q, const uint32_t sig[16], const uint32_t pk[8], const uint8_t* msg,
                         uint64_t mlen) {
  switch (w) {
    case 4: return comb_point<4>(Q, sig, pk, msg, mlen);
    case 5: return comb_point<5>(Q, sig, pk, msg, mlen);
    case 6: return comb_point<6>(Q, sig, pk, msg, mlen);
    case 7: return comb_point<7>(Q, sig, pk, msg, mlen);
    case 9: return comb_point<9>(Q, sig, pk, msg, mlen);
    case 10: return comb_point<10>(Q, sig, pk, msg, mlen);
    case 11: return comb_point<11>(Q, sig, pk, msg, mlen);
    case 12: return comb_point<12>(Q, sig, pk, msg, mlen);
    case 14: return comb_point<14>(Q, sig, pk, msg, mlen);
    case 16: return comb_point<16>(Q, sig, pk, msg, mlen);
    default: return comb_point<8>(Q, sig, pk, msg, mlen);
  }
}

extern "C" {

int edv_host_verify_comb_w(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* msg, uint64_t mlen, int w) {
  uint32_t sig[16], pk[8];
  memcpy(sig, sig64, 64);
  memcpy(pk, pk32, 32);
  ge_p3 Q;
  const bool ok = comb_point_w(w, Q, sig, pk, msg, mlen);
  return (ok && encode_equals(Q, sig)) ? 0 : -1;
}

int edv_host_verify_comb(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* msg, uint64_t mlen) {
  return edv_host_verify_comb_w(sig64, pk32, msg, mlen, 4);
}

}  // extern "C"

template <int W>
static int digits_w(const uint32_t x[8], int* out, bool by_next) {
  if (by_next) {  // the batch kernels' routine: funnel shifts, one digit per call
    CombDigits<W> dg(x);
    for (int r = 0; r < Window<W>::kRows; ++r) out[r] = dg.next();
  } else {
    uint32_t y[9];
    comb_recode<W>(y, x);
    for (int r = 0; r < Window<W>::kRows; ++r) out[r] = comb_digit<W>(y, r);
  }
  return Window<W>::kRows;
}

#define EDV_HOST_WINDOWS(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(24)

static int digits_any(const uint8_t x32[32], int w, int* out, bool by_next) {
  uint32_t x[8];
  memcpy(x, x32, 32);
  switch (w) {
#define EDV_HOST_DIGITS(W) \
  case W: return digits_w<W>(x, out, by_next);
    EDV_HOST_WINDOWS(EDV_HOST_DIGITS)
#undef EDV_HOST_DIGITS
    default: return -1;
  }
}

template <int W>
static int64_t table_w(const ge_p3& P, uint32_t* out) {
  if (out) {
    std::vector<uint32_t> tab;
    build_table<W>(tab, P);
    memcpy(out, tab.data(), tab.size() * 4);
  }
  return (int64_t)Window<W>::kTableWords;
}

extern "C" {

// comb.h signed radix-2^W digits of a 32-byte scalar (W = 4..16 and 24) through comb_digit (the
// small and resident kernels' routine); returns the row count, -1 for another W.
int edv_host_comb_digits(const uint8_t x32[32], int w, int* out) { return digits_any(x32, w, out, false); }
// The same digits through CombDigits<W>::next() (the batch kernels' routine).
int edv_host_comb_digits_next(const uint8_t x32[32], int w, int* out) { return digits_any(x32, w, out, true); }

// The comb table of the point pk32 encodes (negate != 0: of its negative, as the key store holds
// -A) at window w <= 16, built by build_table<W> -- comb_rows and comb_fill_strided lane by lane, as
// edv_key_rows_kernel / edv_comb_fill_kernel run them -- in comb.h's layout (row-major: row r's
// entries at r * 2^(w-1)).  Returns the table's word count (out may be null to ask for it only);
// -1 for another w or an encoding that is not on the curve.
int64_t edv_host_comb_table(const uint8_t pk32[32], int negate, int w, uint32_t* out) {
  uint32_t pk[8];
  memcpy(pk, pk32, 32);
  ge_p3 P;
  if (w < 4 || w > 16 || !ge_frombytes(P, pk, negate != 0)) return -1;
  switch (w) {
#define EDV_HOST_TABLE(W) \
  case W: return W <= 16 ? table_w<(W <= 16 ? W : 16)>(P, out) : -1;
    EDV_HOST_WINDOWS(EDV_HOST_TABLE)
#undef EDV_HOST_TABLE
    default: return -1;
  }
}

}  // extern "C"

// The batched encode (batch_encode.h) over groups of M = 16 consecutive items,
// as edv_encode_kernel runs it per lane.  zero_z[i] != 0 forces item i's Z to
// 0 (exercises the poisoned-group guard).  Bits: 1 = accept.
namespace {
struct HostEncode {
  const std::vector<ge_p3>* Q;
  std::vector<fe>* pre;
  const uint32_t* R;       // 16 words per item (sig)
  const uint8_t* ok;
  uint8_t* bits;
  uint64_t base, n;
  bool valid(int j) const { return base + j < n; }
  void z(int j, fe& f) const { f = (*Q)[base + j].Z; }
  void xy(int j, fe& X, fe& Y) const {
    X = (*Q)[base + j].X;
    Y = (*Q)[base + j].Y;
  }
  void put_pre(int j, const fe& f) const {
    if (valid(j)) (*pre)[base + j] = f;
  }
  void get_pre(int j, fe& f) const {
    if (valid(j)) f = (*pre)[base + j]; else fe_1(f);
  }
  void emit(int j, const uint32_t enc[8], bool zero_z) const {
    if (!valid(j)) return;
    const uint64_t i = base + j;
    const bool acc = !zero_z && ok[i] && memcmp(enc, R + 16 * i, 32) == 0;
    if (acc) bits[i / 8] |= (uint8_t)(1u << (i % 8));
  }
};
}  // namespace

extern "C" {

int edv_host_verify_batch_comb(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* msgs, const uint64_t* off,
                               uint64_t n, int w, const uint8_t* zero_z, uint8_t* bits) {
  std::vector<ge_p3> Q(n);
  std::vector<fe> pre(n);
  std::vector<uint32_t> sig(16 * n);
  std::vector<uint8_t> ok(n);
  memcpy(sig.data(), sig64, 64 * n);
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t pk[8];
    memcpy(pk, pk32 + 32 * i, 32);
    ok[i] = comb_point_w(w, Q[i], &sig[16 * i], pk, msgs + off[i], off[i + 1] - off[i]);
    if (zero_z && zero_z[i]) fe_0(Q[i].Z);
  }
  memset(bits, 0, (n + 7) / 8);
  for (uint64_t g = 0; g < n; g += 16) {
    HostEncode a{&Q, &pre, sig.data(), ok.data(), bits, g, n};
    encode_batch<16>(a);
  }
  return 0;
}

}  // extern "C"

// ---- BLS (bn254.h) on the CPU, for tests/test_bls.py against the oracle.
extern "C" {

// H(m) as 128 G1 bytes
void edv_host_bls_hash(const uint8_t* msg, uint64_t mlen, uint8_t out128[128]) {
  edv::bn::g1 h;
  edv::bn::g1_hash(h, msg, mlen);
  edv::bn::g1_to_bytes(out128, h);
}
// [sk]H(m) (sk 32 big-endian bytes, < r)
void edv_host_bls_sign(const uint8_t sk32[32], const uint8_t* msg, uint64_t mlen, uint8_t out128[128]) {
  uint32_t k[8];
  edv::bn::words_from_be(k, sk32);
  edv::bn::g1 h, s;
  edv::bn::g1_hash(h, msg, mlen);
  edv::bn::g1_mul(s, h, k);
  edv::bn::g1_to_bytes(out128, s);
}
void edv_host_bls_keygen(const uint8_t sk32[32], const uint8_t gen128[128], uint8_t out128[128]) {
  uint32_t k[8];
  edv::bn::words_from_be(k, sk32);
  edv::bn::g2 g, v;
  edv::bn::g2_from_bytes(g, gen128);
  edv::bn::g2_mul(v, g, k);
  edv::bn::g2_to_bytes(out128, v);
}
// the reduced pairing e(P, Q) as 12 Fp values (tower order c0.c0.a, c0.c0.b,
// c0.c1.a, ..., c1.c2.b), 32 big-endian bytes each
int edv_host_bls_pairing(const uint8_t p128[128], const uint8_t q128[128], uint8_t out[384]) {
  using namespace edv::bn;
  g1 P;
  g2 Q;
  g1_from_bytes(P, p128);
  g2_from_bytes(Q, q128);
  if (g1_isinf(P) || g2_isinf(Q)) return -1;
  fp x, y;
  fp2 qx, qy;
  g1_affine(x, y, P);
  g2_affine(qx, qy, Q);
  fp12 f, e;
  fp12_one(f);
  miller_loop_acc(f, x, y, qx, qy);
  final_exp(e, f);
  const fp* c[12] = {&e.c0.c0.a, &e.c0.c0.b, &e.c0.c1.a, &e.c0.c1.b, &e.c0.c2.a, &e.c0.c2.b,
                     &e.c1.c0.a, &e.c1.c0.b, &e.c1.c1.a, &e.c1.c1.b, &e.c1.c2.a, &e.c1.c2.b};
  for (int k = 0; k < 12; ++k) {
    uint32_t w[8];
    fp_to_plain(w, *c[k]);
    words_to_be(out + 32 * k, w);
  }
  return 0;
}
// Bls.verify over wire bytes: 1 accept, 0 reject
int edv_host_bls_verify(const uint8_t sig128[128], const uint8_t* msg, uint64_t mlen, const uint8_t vk128[128],
                        const uint8_t gen128[128]) {
  using namespace edv::bn;
  g1 s, h;
  g2 v, g;
  g1_from_bytes(s, sig128);
  g1_hash(h, msg, mlen);
  g2_from_bytes(v, vk128);
  g2_from_bytes(g, gen128);
  return bls_check(s, h, v, g) ? 1 : 0;
}

}  // extern "C"

// ---- the wave form's program (bls_wave.h) run step by step on the CPU, for tests/test_bls_program.py.
#include "bls_wave.h"
extern "C" {
// Bls.verify over wire bytes through bls_program.h: 1 accept, 0 reject, 2 degenerate (the
// kernel would redo the check on the four-lane form), -1 an input at infinity (rejected by
// the prologue).  vk_n verkeys are summed (verify_multi_sig).
int edv_host_bls_verify_program(const uint8_t sig128[128], const uint8_t* msg, uint64_t mlen, const uint8_t* vk128,
                                uint64_t vk_n, const uint8_t gen128[128]) {
  using namespace edv::bn;
  thread_local fp S[edv::blsp::kSlots];  // per thread: concurrent callers (test workers) never share slots
  for (int k = 0; k < edv::blsp::kConsts; ++k) fp_load(S[edv::blsp::kConstSlot[k]], edv::blsp::kConstVal + 8 * k);
  g1 s, h;
  g2 g, v;
  g1_from_bytes(s, sig128);
  g1_hash(h, msg, mlen);
  g2_from_bytes(g, gen128);
  g2_inf(v);
  for (uint64_t k = 0; k < vk_n; ++k) {
    g2 t;
    g2_from_bytes(t, vk128 + 128 * k);
    g2_add(v, v, t);
  }
  if (g1_isinf(s) || g2_isinf(g) || g2_isinf(v) || g1_isinf(h)) return -1;
  namespace P = edv::blsp;
  S[P::kIn_xP1] = s.X;
  S[P::kIn_yP1] = s.Y;
  S[P::kIn_xP2] = h.X;
  S[P::kIn_yP2] = h.Y;
  const fp* q[12] = {&g.X.a, &g.X.b, &g.Y.a, &g.Y.b, &g.Z.a, &g.Z.b, &v.X.a, &v.X.b, &v.Y.a, &v.Y.b, &v.Z.a, &v.Z.b};
  const int qs[12] = {P::kIn_Q1Xa, P::kIn_Q1Xb, P::kIn_Q1Ya, P::kIn_Q1Yb, P::kIn_Q1Za, P::kIn_Q1Zb,
                      P::kIn_Q2Xa, P::kIn_Q2Xb, P::kIn_Q2Ya, P::kIn_Q2Yb, P::kIn_Q2Za, P::kIn_Q2Zb};
  for (int k = 0; k < 12; ++k) S[qs[k]] = *q[k];
  uint32_t flag = 0;
  thread_local fp res[64];
  bool wr[64];
  uint32_t dst[64];
  for (int st = 0; st < P::kSteps; ++st) {
    const uint32_t o0 = P::kStep[st], o1 = P::kStep[st + 1];
    for (uint32_t o = o0; o < o1; ++o) {  // every lane reads ...
      const uint32_t* w = P::kOp + (size_t)P::kOpWords * o;
      wr[o - o0] = blsp_exec(w, S, res[o - o0], &flag);
      dst[o - o0] = blsp_field(w, 0);
    }
    for (uint32_t o = o0; o < o1; ++o)  // ... then every lane writes
      if (wr[o - o0]) S[dst[o - o0]] = res[o - o0];
  }
  if (flag) return 2;
  return blsp_result_is_one(S) ? 1 : 0;
}

// create_multi_sig over wire bytes: the sum of n G1 points (edv_bls_aggregate_kernel's loop)
void edv_host_bls_aggregate(const uint8_t* sig128, uint64_t n, uint8_t out128[128]) {
  using namespace edv::bn;
  g1 acc;
  g1_inf(acc);
  for (uint64_t k = 0; k < n; ++k) {
    g1 t;
    g1_from_bytes(t, sig128 + 128 * k);
    g1_add(acc, acc, t);
  }
  g1_to_bytes(out128, acc);
}

// The CPU twins of tests/native/bls_fp_probe.hip (same signatures): the Fp primitives on raw
// 8-limb values below p, and single program operations over a slot table.
// op: 0 fp_add, 1 fp_sub, 2 fp_neg, 3 fp_dbl, 4 fp_mul, 5 fp_inv_plain_vt (neg, dbl, inv: of a)
int edv_host_bn_fp(int op, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  using namespace edv::bn;
  if (op < 0 || op > 5) return -1;
  for (uint64_t i = 0; i < n; ++i) {
    fp x, y, r;
    fp_load(x, a + 8 * i);
    fp_load(y, b + 8 * i);
    switch (op) {
      case 0: fp_add(r, x, y); break;
      case 1: fp_sub(r, x, y); break;
      case 2: fp_neg(r, x); break;
      case 3: fp_dbl(r, x); break;
      case 4: fp_mul(r, x, y); break;
      default: fp_inv_plain_vt(r.v, x.v); break;
    }
    for (int k = 0; k < 8; ++k) out[8 * i + k] = r.v[k];
  }
  return 0;
}
// ops: n_ops x kOpWords words; slots: n_slots x 8 limbs (read only); per operation out (8 limbs,
// zero when nothing is written), wrote (blsp_exec's return) and flag.  -1: a field names a slot
// past the table.
int edv_host_blsp_exec(const uint32_t* ops, uint64_t n_ops, const uint32_t* slots, uint64_t n_slots, uint32_t* out,
                       uint8_t* wrote, uint32_t* flag) {
  using namespace edv::bn;
  namespace P = edv::blsp;
  for (uint64_t i = 0; i < n_ops; ++i)
    for (int f = 0; f <= P::kMaxTerms; ++f)
      if (blsp_field(ops + P::kOpWords * i, f) >= n_slots) return -1;
  const fp* S = (const fp*)slots;
  for (uint64_t i = 0; i < n_ops; ++i) {
    fp r;
    fp_zero(r);
    uint32_t fl = 0;
    wrote[i] = blsp_exec(ops + P::kOpWords * i, S, r, &fl) ? 1 : 0;
    flag[i] = fl;
    for (int k = 0; k < 8; ++k) out[8 * i + k] = r.v[k];
  }
  return 0;
}
// kOpWords, kMaxTerms, then the kind codes kNop, kMul, kInv, kZchk, kLin
void edv_host_blsp_layout(uint32_t out[7]) {
  namespace P = edv::blsp;
  const uint32_t v[7] = {(uint32_t)P::kOpWords, (uint32_t)P::kMaxTerms, P::kNop, P::kMul, P::kInv, P::kZchk, P::kLin};
  for (int k = 0; k < 7; ++k) out[k] = v[k];
}
}  // extern "C"

// ---- the wire scanner (wire_scan.h, the code of edv_wire_scan_kernel's lanes) on the CPU, every
// read and write of it asserted inside the item's text / output span, for tests/test_wire_scan.py.
#include "wire_scan.h"
namespace {
struct CheckedText {
  const uint8_t* p;
  uint32_t n;
  uint8_t operator[](uint32_t i) const {
    EDV_ASSERT(i < n);
    return p[i];
  }
};
struct CheckedOut {
  uint8_t* p;
  uint32_t n;
  uint8_t& operator[](uint32_t i) const {
    EDV_ASSERT(i < n);
    return p[i];
  }
};
}  // namespace
extern "C" {
// n texts (item i = text[off[i] .. off[i + 1])): status[n] (0 scanned, 1 the host decides),
// idr_span[2n] (start, length; zero where status != 0), sig64[64n], msg_len[n], and item i's
// serialization at msgs[off[i] - off[0] ..) (msgs holds off[n] - off[0] bytes).
void hc_wire_scan(const uint8_t* text, const uint64_t* off, uint64_t n, uint8_t* status, uint32_t* idr_span,
                  uint8_t* sig64, uint8_t* msgs, uint32_t* msg_len) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = off[i + 1] - off[i];
    WireItem it;
    memset(&it, 0, sizeof it);
    int st = kWireHost;
    if (len <= kWireMaxText) {
      const CheckedText t{text + off[i], (uint32_t)len};
      const CheckedOut o{msgs + (off[i] - off[0]), (uint32_t)len};
      st = wire_scan_one(t, (uint32_t)len, o, it);
    }
    status[i] = (uint8_t)st;
    const bool ok = st == kWireOk;
    idr_span[2 * i] = ok ? it.idr_start : 0;
    idr_span[2 * i + 1] = ok ? it.idr_len : 0;
    msg_len[i] = ok ? it.msg_len : 0;
    if (ok)
      memcpy(sig64 + 64 * i, it.sig, 64);
    else
      memset(sig64 + 64 * i, 0, 64);
  }
}
}  // extern "C"

// ---- the node-message unwrap (wire_unwrap.h, the code of edv_wire_unwrap_kernel's lanes) on the
// CPU, every read and write asserted inside the message's own span, for tests/test_wire_unwrap.py.
#include "wire_unwrap.h"
extern "C" {
// n messages (message i = text[off[i] .. off[i + 1]), esc[i] = 1: a JSON string body): cls[n]
// (0 request, 1 the host decides, 2 no signed request) and message i's unwrapped text at
// out[off[i] - off[0] ..) (out holds off[n] - off[0] bytes; spaces for a message over kWireMaxText,
// which the lane code leaves unread).
void hc_wire_unwrap(const uint8_t* text, const uint64_t* off, const uint8_t* esc, uint64_t n, uint8_t* cls,
                    uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = off[i + 1] - off[i];
    uint8_t* o = out + (off[i] - off[0]);
    if (len > kWireMaxText) {
      memset(o, ' ', (size_t)len);
      cls[i] = (uint8_t)kUnwrapHost;
      continue;
    }
    cls[i] = (uint8_t)wire_unwrap_one(CheckedText{text + off[i], (uint32_t)len}, (uint32_t)len, esc[i],
                                      CheckedOut{o, (uint32_t)len});
  }
}
}  // extern "C"

// ---- the wire batch's distinct identifiers (wire_idents.h, the code of edv_wire_ident_*_kernel's
// lanes) on the CPU, every read and write asserted in bounds, for tests/test_wire_idents.py.
#include "wire_idents.h"
namespace {
template <class V>
struct CheckedArr {
  V* p;
  uint64_t n;
  V& operator[](uint64_t i) const {
    EDV_ASSERT(i < n);
    return p[i];
  }
};
struct CheckedBytes {  // the texts, by their position in the caller's buffer
  const uint8_t* p;
  uint64_t lo, hi;
  uint8_t operator[](uint64_t i) const {
    EDV_ASSERT(i >= lo && i < hi);
    return p[i];
  }
};
struct SerialTable {  // the device's atomics, one item at a time
  CheckedArr<uint32_t> owner, first;
  uint32_t owner_load(uint32_t s) const { return owner[s]; }
  uint32_t owner_cas(uint32_t s, uint32_t i) const {
    const uint32_t was = owner[s];
    if (was == kIdentEmpty) owner[s] = i;
    return was;
  }
  uint32_t first_load(uint32_t s) const { return first[s]; }
  void first_min(uint32_t s, uint32_t i) const {
    if (i < first[s]) first[s] = i;
  }
};
}  // namespace
extern "C" {
// The distinct identifiers of the status-0 items of n texts (item i = text[off[i] .. off[i + 1]),
// identifier span[2i], span[2i + 1] inside it), the items inserted in the order order[0 .. n) (a
// permutation) into a table of cap slots (a power of two, at least the number of identifiers):
// uidx[n] = the item's index among the identifiers in first-occurrence order (nu elsewhere),
// uniq_item[0 .. nu) = each identifier's first item.  Returns nu; -1 a span outside its item (no
// byte outside the texts is read), -2 a table that is too small or not a power of two.
int64_t hc_wire_idents(const uint8_t* text, const uint64_t* off_p, uint64_t n, const uint8_t* status_p,
                       const uint32_t* span_p, uint64_t cap, const uint32_t* order_p, uint32_t* uidx_p,
                       uint32_t* uniq_item_p) {
  if (cap == 0 || (cap & (cap - 1)) || cap > 0x80000000ull) return -2;
  const CheckedArr<const uint64_t> off{off_p, n + 1};
  const CheckedArr<const uint8_t> status{status_p, n};
  const CheckedArr<const uint32_t> span{span_p, 2 * n}, order{order_p, n};
  const CheckedArr<uint32_t> uidx{uidx_p, n}, uniq_item{uniq_item_p, n};
  const CheckedBytes t{text, off[0], off[n]};
  std::vector<uint32_t> owner_v((size_t)cap, kIdentEmpty), first_v((size_t)cap, kIdentEmpty);
  std::vector<uint32_t> slot_v((size_t)n + 1, kIdentEmpty), flag_v((size_t)n + 1, 0), rank_v((size_t)n + 1, 0);
  const SerialTable tab{{owner_v.data(), cap}, {first_v.data(), cap}};
  const CheckedArr<uint32_t> slot{slot_v.data(), n}, flag{flag_v.data(), n + 1}, rank{rank_v.data(), n + 1};
  bool bad = false, full = false;
  for (uint64_t k = 0; k < n; ++k) {
    const uint32_t i = order[k];
    if (status[i] != 0) continue;
    if (!wi_span_ok(off, span, i)) {
      bad = true;
      continue;
    }
    slot[i] = wi_insert(t, off, span, tab, (uint32_t)cap, i);
    full |= slot[i] == kIdentEmpty;
  }
  if (bad) return -1;
  if (full) return -2;
  for (uint64_t i = 0; i < n; ++i) flag[i] = wi_flag(slot, tab.first, i);
  for (uint64_t i = 0; i < n; ++i) rank[i + 1] = rank[i] + flag[i];
  for (uint64_t i = 0; i < n; ++i) {
    uidx[i] = wi_index(slot, tab.first, rank, n, i);
    if (flag[i]) uniq_item[rank[i]] = (uint32_t)i;
  }
  return (int64_t)rank[n];
}
}  // extern "C"

// ---- the wire batch's work list (wire_once.h, the code of edv_wire_once_*_kernel's lanes) on the
// CPU, every read and write asserted in bounds, for tests/test_wire_once.py and the list double.
#include "wire_once.h"
namespace {
struct CheckedMsg {  // the serializations; word64 at any byte position, wholly inside them
  const uint8_t* p;
  uint64_t n;
  uint8_t operator[](uint64_t i) const {
    EDV_ASSERT(i < n);
    return p[i];
  }
  uint64_t word64(uint64_t i) const {
    EDV_ASSERT(i <= n && n - i >= 8);
    uint64_t v;
    memcpy(&v, p + i, 8);
    return v;
  }
};
}  // namespace
extern "C" {
// The work list of n items: signatures sig64[64 n] (4-byte aligned), message i =
// msgs[spans[i] .. spans[n + i]) inside msg_bytes bytes, status[n], uidx[n] (nu for an item without
// an identifier), kid_u[nu] (a key id, 0xffffffff general, 0xfffffffe skip).  once: the live items
// are inserted in the order order[0 .. n) (a permutation) into a table of cap slots (a power of
// two), each passing at most `probe` slots.  rep[n] = the item whose verdict the item takes (itself
// for a dead one), grp[n] = 0 dead, 1 keyed, 2 general; *give_ups = the live items that found no
// slot, *longest_run = the longest run of occupied slots (around the end; cap for a full table).
// Returns the number of lanes (live items that are their own representative); -1 a message span
// outside msg_bytes (no byte outside is read), -2 cap not a power of two.
int64_t hc_wire_once(const uint8_t* sig64, const uint8_t* msgs, uint64_t msg_bytes, const uint64_t* spans_p, uint64_t n,
                     const uint8_t* status_p, const uint32_t* uidx_p, const uint32_t* kid_p, uint64_t nu, uint32_t once,
                     uint64_t cap, uint32_t probe, const uint32_t* order_p, uint32_t* rep_p, uint8_t* grp_p,
                     uint64_t* give_ups, uint64_t* longest_run) {
  if (cap == 0 || (cap & (cap - 1)) || cap > 0x80000000ull) return -2;
  const CheckedArr<const uint32_t> sigw{(const uint32_t*)sig64, 16 * n}, uidx{uidx_p, n}, kid{kid_p, nu}, order{order_p, n};
  const CheckedArr<const uint64_t> ms{spans_p, n}, me{spans_p + n, n};
  const CheckedArr<const uint8_t> status{status_p, n};
  const CheckedArr<uint32_t> rep{rep_p, n};
  const CheckedArr<uint8_t> grp{grp_p, n};
  const CheckedMsg msg{msgs, msg_bytes};
  std::vector<uint32_t> owner_v((size_t)cap, kIdentEmpty), first_v((size_t)cap, kIdentEmpty), slot_v((size_t)n + 1, kIdentEmpty);
  const SerialTable tab{{owner_v.data(), cap}, {first_v.data(), cap}};
  const CheckedArr<uint32_t> slot{slot_v.data(), n};
  bool bad = false;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t g = wo_group(status, uidx, kid, (uint32_t)nu, i);
    if (g != kOnceDead && !wo_span_ok(ms, me, msg_bytes, i)) {
      g = kOnceDead;
      bad = true;
    }
    grp[i] = (uint8_t)g;
  }
  if (bad) return -1;
  uint64_t gave = 0;
  for (uint64_t k = 0; k < n && once; ++k) {
    const uint32_t i = order[k];
    if (grp[i] == kOnceDead) continue;
    slot[i] = wo_insert(sigw, ms, me, msg, uidx, tab, (uint32_t)cap, probe, i);
    gave += (uint64_t)(slot[i] == kIdentEmpty);
  }
  int64_t lanes = 0;
  for (uint64_t i = 0; i < n; ++i) {
    rep[i] = wo_rep(slot, tab.first, i);
    lanes += (int64_t)(wo_flag(grp, slot, tab.first, kOnceKeyed, i) + wo_flag(grp, slot, tab.first, kOnceGeneral, i));
  }
  uint64_t run = 0, longest = 0, occupied = 0;
  for (uint64_t s = 0; s < 2 * cap; ++s) {  // (twice around: a run over the end)
    run = owner_v[(size_t)(s & (cap - 1))] != kIdentEmpty ? run + 1 : 0;
    if (run > longest) longest = run;
  }
  for (uint64_t s = 0; s < cap; ++s) occupied += (uint64_t)(owner_v[(size_t)s] != kIdentEmpty);
  if (give_ups) *give_ups = gave;
  if (longest_run) *longest_run = occupied == cap ? cap : longest;
  return lanes;
}
}  // extern "C"

// ---- the wire batch's request digests (wire_digest.h, the code of edv_wire_digest_kernel's lanes)
// on the CPU, every read of the walk asserted inside the item's text, for tests/test_wire_digest.py
// and the digest double.
#include "wire_digest.h"
extern "C" {
// wd_eligible over text[at .. at + len) alone (the accessor asserts every read inside it).
uint32_t hc_wd_eligible(const uint8_t* text, uint64_t at, uint32_t len) {
  return wd_eligible(CheckedBytes{text, at, at + len}, at, len);
}

// n texts (item i = text[off[i] .. off[i + 1])) with what hc_wire_scan made of them: status[n] and
// item i's serialization msgs[off[i] - off[0] ..)[: msg_len[i]].  have[n] and digest32[32 n] as
// edv_wire_digests returns them: 1 and sha256(serialization) for a status-0 item that wd_eligible
// accepts, 0 and a zero row for every other item.
void hc_wire_digests(const uint8_t* text, const uint64_t* off_p, uint64_t n, const uint8_t* status_p,
                     const uint8_t* msgs, const uint32_t* msg_len_p, uint8_t* digest32, uint8_t* have_p) {
  const CheckedArr<const uint64_t> off{off_p, n + 1};
  const CheckedArr<const uint8_t> status{status_p, n};
  const CheckedArr<const uint32_t> msg_len{msg_len_p, n};
  const CheckedArr<uint8_t> have{have_p, n}, dig{digest32, 32 * n};
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t a = off[i], len = off[i + 1] - off[i];
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t ok = 0;
    if (status[i] == 0 && len <= kWireMaxText) ok = wd_eligible(CheckedBytes{text, a, a + len}, a, (uint32_t)len);
    if (ok) {
      EDV_ASSERT(msg_len[i] <= len);
      alignas(16) uint8_t m[kWireMaxText + 16];  // (sha256_msg reads whole aligned 16-byte pieces)
      memset(m, 0, sizeof m);
      memcpy(m, msgs + (a - off[0]), msg_len[i]);
      sha256_msg(d, m, msg_len[i]);
    }
    for (int k = 0; k < 32; ++k) dig[32 * i + k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
    have[i] = (uint8_t)ok;
  }
}
}  // extern "C"

// ---- the device BATCH split (node_split_lanes.h, the code of edv_node_split_count_kernel's and
// edv_node_split_emit_kernel's lanes) on the CPU as an emulated wave: 64 lanes one after the other,
// the same Hillis-Steele composition the shuffles do and the same carry from step to step; every
// read asserted inside the entry, every write inside the outputs.  For tests/test_node_split_lanes.py
// and the node wire double.
#include "node_split_wave_host.h"
namespace {
struct CheckedEntry {
  const uint8_t* p;
  uint64_t n;
  uint8_t operator[](uint64_t i) const {
    EDV_ASSERT(i < n);
    return p[i];
  }
};

}  // namespace
extern "C" {
// The messages of n_e entries (entry e = text[entry_off[e] .. entry_off[e + 1])) as the two device
// passes make them.  Returns m, the number of messages, and their bytes in *n_bytes.  With off null
// that is all (pass A and the sums); otherwise cap >= m and off[m + 1] (from 0), esc[m], entry[m],
// at[m] (the position of the message's first byte in text) are written (pass B).
int64_t hc_node_split_lanes(const uint8_t* text, const uint64_t* entry_off, uint64_t n_e, uint64_t cap, uint64_t* off_p,
                            uint8_t* esc_p, uint32_t* entry_p, uint64_t* at_p, uint64_t* n_bytes) {
  const uint64_t base = n_e ? entry_off[0] : 0;
  std::vector<EntryCount> count((size_t)n_e);
  std::vector<uint64_t> msg0((size_t)n_e + 1, 0), body0((size_t)n_e + 1, 0);
  for (uint64_t e = 0; e < n_e; ++e) {
    EDV_ASSERT(entry_off[e] <= entry_off[e + 1]);
    const CheckedEntry t{text + entry_off[e], entry_off[e + 1] - entry_off[e]};
    count[e] = lanes_count(t, entry_off[e] - base, entry_off[e + 1] - base);
    msg0[e + 1] = msg0[e] + count[e].members;
    body0[e + 1] = body0[e] + count[e].bytes;
  }
  const uint64_t m = msg0[n_e];
  *n_bytes = body0[n_e];
  if (!off_p) return (int64_t)m;
  EDV_ASSERT(cap >= m);
  const CheckedArr<uint64_t> off{off_p, m + 1}, at{at_p, m};
  const CheckedArr<uint8_t> esc{esc_p, m};
  const CheckedArr<uint32_t> entry{entry_p, m};
  off[m] = body0[n_e];
  for (uint64_t e = 0; e < n_e; ++e) {
    const uint64_t k0 = msg0[e], k1 = msg0[e + 1], b0 = body0[e];
    if (!count[e].split) {
      off[k0] = b0;
      esc[k0] = 0;
      entry[k0] = (uint32_t)e;
      at[k0] = entry_off[e];
      continue;
    }
    const CheckedEntry t{text + entry_off[e], entry_off[e + 1] - entry_off[e]};
    lanes_emit(t, entry_off[e] - base, entry_off[e + 1] - base, [&](uint64_t index, uint64_t body, uint64_t first) {
      EDV_ASSERT(k0 + index < k1);
      off[k0 + index] = b0 + body;
      esc[k0 + index] = 1;
      entry[k0 + index] = (uint32_t)e;
      at[k0 + index] = base + first;
    });
  }
  return (int64_t)m;
}
}  // extern "C"

// ---- the CPU twins of tests/native/ed_probe.hip's one-item-per-lane entry points (same
// signatures, the same calls: csrc/ed_probe_ops.h), for tests/test_ed_edges.py: the tables of
// tests/ed_edge_common.py through this build's EDV_BOUND_CHECK assertions.
#include <stdlib.h>

#include "ed_probe_ops.h"
extern "C" {
// the base comb's window in this build (kBaseW)
int edv_host_ed_base_w(void) { return edv::kBaseW; }
int edv_host_ed_lane_io(int op, int io[2]) {
  if (op < 0 || op >= edv::edp::kLaneOps) return -1;
  io[0] = edv::edp::lane_in_words(op);
  io[1] = edv::edp::lane_out_words(op);
  return 0;
}
int edv_host_ed_lane(int op, const uint32_t* in, uint64_t n, uint32_t* out) {
  namespace P = edv::edp;
  if (op < 0 || op >= P::kLaneOps || n > 0x7fffffffull) return -1;
  if (op == P::kFeSqn)
    for (uint64_t i = 0; i < n; ++i)
      if (in[11 * i + 10] < 1 || in[11 * i + 10] > 300) return -1;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t* a = in + (uint64_t)P::lane_in_words(op) * i;
    uint32_t* o = out + (uint64_t)P::lane_out_words(op) * i;
    switch (op) {
#define EDV_CASE(OP) \
  case OP: P::lane_op<OP>(a, o); break;
      EDV_ED_LANE_OPS(EDV_CASE)
#undef EDV_CASE
    }
  }
  return 0;
}
// forms 0 and 1 (the wave form is device only: -1)
int edv_host_ed_hash(int form, const uint8_t* sig64, const uint8_t* pk32, const uint8_t* buf, uint64_t buf_len,
                     const uint64_t* start, const uint64_t* mlen, uint64_t n, uint32_t* h_out, uint8_t* ok_out) {
  if (form < 0 || form > 1) return -1;
  for (uint64_t i = 0; i < n; ++i)
    if (start[i] > buf_len || mlen[i] > buf_len - start[i]) return -1;
  const size_t padded = (buf_len + 15) / 16 * 16 + 16;
  uint8_t* b = (uint8_t*)aligned_alloc(16, padded);  // start[i] mod 16 is the message's alignment
  if (!b) return -2;
  memset(b, 0, padded);
  memcpy(b, buf, buf_len);
  std::vector<Chunk16> units;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t sig[16], pk[8], h[8];
    memcpy(sig, sig64 + 64 * i, 64);
    memcpy(pk, pk32 + 32 * i, 32);
    units.assign(sha512_units64(mlen[i]), Chunk16{0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu});
    ok_out[i] = edv::edp::hash_op(form, h, sig, pk, b + start[i], mlen[i], units.data()) ? 1 : 0;
    memcpy(h_out + 8 * i, h, 32);
  }
  free(b);
  return 0;
}
// the dedupe of edprobe_dedup with the requests taken one after the other (key_dedup.h's host
// build: plain loads and stores)
int edv_host_ed_dedup(const uint8_t* pk32, uint64_t n, uint64_t nslots, uint32_t* slots, uint32_t* req_slot,
                      uint32_t* slot_u, uint32_t* reps, uint32_t* count, uint32_t* hashes, int* split) {
  if (!edv::edp::dedup_args_ok(n, nslots)) return -1;
  uint8_t* keys = (uint8_t*)aligned_alloc(16, 32 * n);
  if (!keys) return -2;
  memcpy(keys, pk32, 32 * n);
  memset(slots, 0xff, 4 * nslots);
  memset(req_slot, 0xff, 4 * n);
  memset(slot_u, 0xff, 4 * nslots);
  memset(reps, 0xff, 4 * n);
  *count = 0;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t pk[8];
    edv::load_key(pk, keys, i);
    hashes[i] = edv::key_hash(pk);
    edv::dedup_insert(keys, i, slots, (uint32_t)nslots, req_slot);
  }
  for (uint64_t i = 0; i < n; ++i) edv::dedup_assign(i, slots, req_slot, slot_u, reps, count);
  *split = edv::split_of(*count, n);
  free(keys);
  return 0;
}
}  // extern "C"
