// bls_fp_probe.hip -- TEST ONLY: the BLS wave form's Fp primitives (csrc/bn254.h,
// csrc/bls_wave.h) one item per lane, for tests/test_gpu_bls_fp.py against Python
// integers.  Built as libedv_bls_probe.so; the package never loads it.  The host
// twins with the same signatures are edv_host_bn_fp / edv_host_blsp_exec /
// edv_host_blsp_layout (csrc/host_check.cpp).
//
// Host-pointer entry points: each allocates, launches one kernel (block 64), copies
// back and returns the HIP error code (0 = hipSuccess); -1 for an argument the
// kernel must not see (an unknown op, a slot index past the table).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../indy-plenum_amd/csrc/bls_wave.h"

using namespace edv::bn;
namespace blsp = edv::blsp;

namespace {

constexpr int kBlock = 64;

__global__ __launch_bounds__(kBlock) void blsprobe_fp_kernel(int op, const uint32_t* __restrict__ a,
                                                            const uint32_t* __restrict__ b, uint64_t n,
                                                            uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
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
#pragma unroll
  for (int k = 0; k < 8; ++k) out[8 * i + k] = r.v[k];
}

__global__ __launch_bounds__(kBlock) void blsprobe_exec_kernel(const uint32_t* __restrict__ ops, uint64_t n_ops,
                                                              const fp* __restrict__ slots, uint32_t* __restrict__ out,
                                                              uint8_t* __restrict__ wrote, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ops) return;
  uint32_t w[blsp::kOpWords];
#pragma unroll
  for (int k = 0; k < blsp::kOpWords; ++k) w[k] = ops[blsp::kOpWords * i + k];
  fp r;
  fp_zero(r);
  uint32_t fl = 0;
  const bool wr = blsp_exec(w, slots, r, &fl);
  wrote[i] = wr ? 1 : 0;
  flag[i] = fl;
#pragma unroll
  for (int k = 0; k < 8; ++k) out[8 * i + k] = r.v[k];
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
};

#define PROBE_TRY(expr)              \
  do {                               \
    hipError_t e_ = (expr);          \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

}  // namespace

extern "C" {

// op: 0 fp_add, 1 fp_sub, 2 fp_neg, 3 fp_dbl, 4 fp_mul, 5 fp_inv_plain_vt (neg, dbl, inv: of a);
// a, b, out: n x 8 limbs, raw values below p
int blsprobe_fp(int op, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  if (op < 0 || op > 5) return -1;
  if (n == 0) return 0;
  Bufs bufs;
  void *d_a, *d_b, *d_out;
  PROBE_TRY(bufs.alloc(&d_a, 32 * n));
  PROBE_TRY(bufs.alloc(&d_b, 32 * n));
  PROBE_TRY(bufs.alloc(&d_out, 32 * n));
  PROBE_TRY(hipMemcpy(d_a, a, 32 * n, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_b, b, 32 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(blsprobe_fp_kernel, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, op,
                     (const uint32_t*)d_a, (const uint32_t*)d_b, n, (uint32_t*)d_out);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(out, d_out, 32 * n, hipMemcpyDeviceToHost));
  return 0;
}

// Each lane runs blsp_exec on its own operation (ops: n_ops x kOpWords words) over the shared,
// read-only slot table (slots: n_slots x 8 limbs).  Per operation: out (8 limbs, zero when nothing
// is written), wrote (blsp_exec's return) and flag.
int blsprobe_exec(const uint32_t* ops, uint64_t n_ops, const uint32_t* slots, uint64_t n_slots, uint32_t* out,
                  uint8_t* wrote, uint32_t* flag) {
  for (uint64_t i = 0; i < n_ops; ++i)  // every field an operation can read stays inside the table
    for (int f = 0; f <= blsp::kMaxTerms; ++f)
      if (blsp_field(ops + blsp::kOpWords * i, f) >= n_slots) return -1;
  if (n_ops == 0) return 0;
  Bufs bufs;
  void *d_ops, *d_slots, *d_out, *d_wrote, *d_flag;
  PROBE_TRY(bufs.alloc(&d_ops, 4 * blsp::kOpWords * n_ops));
  PROBE_TRY(bufs.alloc(&d_slots, 32 * n_slots));
  PROBE_TRY(bufs.alloc(&d_out, 32 * n_ops));
  PROBE_TRY(bufs.alloc(&d_wrote, n_ops));
  PROBE_TRY(bufs.alloc(&d_flag, 4 * n_ops));
  PROBE_TRY(hipMemcpy(d_ops, ops, 4 * blsp::kOpWords * n_ops, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_slots, slots, 32 * n_slots, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(blsprobe_exec_kernel, dim3((uint32_t)((n_ops + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0,
                     (const uint32_t*)d_ops, n_ops, (const fp*)d_slots, (uint32_t*)d_out, (uint8_t*)d_wrote,
                     (uint32_t*)d_flag);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipMemcpy(out, d_out, 32 * n_ops, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(wrote, d_wrote, n_ops, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(flag, d_flag, 4 * n_ops, hipMemcpyDeviceToHost));
  return 0;
}

// kOpWords, kMaxTerms, then the kind codes kNop, kMul, kInv, kZchk, kLin
void blsprobe_layout(uint32_t out[7]) {
  const uint32_t v[7] = {(uint32_t)blsp::kOpWords, (uint32_t)blsp::kMaxTerms, blsp::kNop, blsp::kMul,
                         blsp::kInv,               blsp::kZchk,               blsp::kLin};
  for (int k = 0; k < 7; ++k) out[k] = v[k];
}

}  // extern "C"
