// Fused SGD with momentum over the flat fp32 parameter buffer (one launch for all parameters).
//
// Replaces torch.optim.SGD(params_list, lr, momentum=config.momentum, weight_decay=config.weight_decay)
// (config.optimizer == 'SGDM', train.py:116-117,130-131) with the two param groups of
// utils/init_func.py:group_weight, using torch.optim.SGD's single-tensor update order with
// dampening = 0:
//   g1 = g * s ; g1 += wd * p (decay group) ; buf = mu * buf + g1
//   d = nesterov ? g1 + mu * buf : buf ; p -= lr * d
// s = grad_scale / loss_scale[0] (the 1/P data-parallel fold and GradScaler's unscale).  wd and mu
// arrive as doubles and are rounded to fp32 once, as torch rounds its Python-float scalars.  Before
// the first step buf is zero, and 0 * mu + g1 is torch's first-step buf = clone(g1) bit for bit.
// lr is read from device memory so the step can be replayed from a HIP graph while WarmUpPolyLR
// changes lr.  The per-64-element flag is adamw.hip's (1 = decay, 0 = none, 2 = frozen: untouched);
// found_inf[0] != 0 skips the whole step (p, buf and the shadow keep their bits).  Optionally emits
// the 16-bit weight shadow for the next step's GEMMs.
// HBM-bound: 12 B read (p,g,buf) + 8 B written (p,buf) [+2 B shadow] per parameter; momentum = 0 is
// an instance of its own that never touches buf: 8 B read + 4 B written [+2 B].
// No step count, so no tickets and no atomics: every block is independent.
#include "cmx_common.h"

// NT = nontemporal (streaming) loads and stores: every byte is touched once per step
typedef float sgdm_f4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 sgdm_ld4(const float* a) {
  if constexpr (NT) {
    const sgdm_f4 t = __builtin_nontemporal_load(reinterpret_cast<const sgdm_f4*>(a));
    return make_float4(t.x, t.y, t.z, t.w);
  } else {
    return *reinterpret_cast<const float4*>(a);
  }
}
template <bool NT>
__device__ __forceinline__ void sgdm_st4(float* a, float x, float y, float z, float w) {
  if constexpr (NT) __builtin_nontemporal_store((sgdm_f4){x, y, z, w}, reinterpret_cast<sgdm_f4*>(a));
  else *reinterpret_cast<float4*>(a) = make_float4(x, y, z, w);
}

// S = the weight shadow's 16-bit type; MOM = momentum != 0 (buf is read and written)
template <typename S, bool NT, bool MOM>
__global__ __launch_bounds__(256) void sgdm_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ buf, S* __restrict__ shadow,
                                                   const uint8_t* __restrict__ decay64, long n,
                                                   const float* __restrict__ lr_ptr, float mu, float wd, int nesterov,
                                                   float gscale_in, const float* __restrict__ loss_scale,
                                                   const float* __restrict__ found_inf) {
  // GradScaler semantics (train.py:185-198): a step whose gradients held inf / nan is skipped
  if (found_inf && *found_inf != 0.f) return;
  const float lr = *lr_ptr;
  const float gscale = loss_scale ? gscale_in / *loss_scale : gscale_in;       // unscale
  const long nv = n / 4;
  auto update = [&](const long e, const float4 pp, const float4 gg, const float4 bb, const uint8_t flag) {
    if (flag == 2) return;                             // 0: no decay, 1: decay, 2: frozen
    float pa[4] = {pp.x, pp.y, pp.z, pp.w}, ga[4] = {gg.x, gg.y, gg.z, gg.w};
    float ba[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gj = ga[j] * gscale;
      if (flag) gj = gj + wd * pa[j];
      float d = gj;
      if constexpr (MOM) {
        ba[j] = mu * ba[j] + gj;
        d = nesterov ? gj + mu * ba[j] : ba[j];
      }
      pa[j] = pa[j] - lr * d;
    }
    sgdm_st4<NT>(p + e, pa[0], pa[1], pa[2], pa[3]);
    if constexpr (MOM) sgdm_st4<NT>(buf + e, ba[0], ba[1], ba[2], ba[3]);
    if (shadow) *reinterpret_cast<uint2*>(shadow + e) = make_uint2(pack2<S>(pa[0], pa[1]), pack2<S>(pa[2], pa[3]));
  };
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  // two float4 groups per thread per iteration: six 16-B loads in flight before any update
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < nv; i += 2 * stride) {
    const long e0 = i * 4, e1 = (i + stride) * 4;
    const float4 p0 = sgdm_ld4<NT>(p + e0), p1 = sgdm_ld4<NT>(p + e1);
    const float4 g0 = sgdm_ld4<NT>(g + e0), g1 = sgdm_ld4<NT>(g + e1);
    float4 b0 = zero, b1 = zero;
    if constexpr (MOM) {
      b0 = sgdm_ld4<NT>(buf + e0);
      b1 = sgdm_ld4<NT>(buf + e1);
    }
    const uint8_t f0 = decay64[e0 >> 6], f1 = decay64[e1 >> 6];
    update(e0, p0, g0, b0, f0);
    update(e1, p1, g1, b1, f1);
  }
  if (i < nv) {
    const long e = i * 4;
    float4 b = zero;
    if constexpr (MOM) b = sgdm_ld4<NT>(buf + e);
    update(e, sgdm_ld4<NT>(p + e), sgdm_ld4<NT>(g + e), b, decay64[e >> 6]);
  }
}

extern "C" {

// n must be a multiple of 64; buf is NULL exactly when momentum == 0; every refusal precedes the
// launch; no allocation and no sync, so the call can be captured into a HIP graph
int cmx_sgdm_step(float* p, const float* g, float* buf, void* shadow, int shadow_dtype, const uint8_t* decay64,
                  int64_t n, const float* lr_ptr, double momentum, double weight_decay, int nesterov, float grad_scale,
                  const float* loss_scale, const float* found_inf, int max_blocks, hipStream_t s) {
  CMX_REQUIRE(n >= 0 && n % 64 == 0, CMX_ERR_SHAPE, "sgdm: n must be a non-negative multiple of 64");
  CMX_REQUIRE(momentum >= 0.0 && weight_decay >= 0.0, CMX_ERR_ARG, "sgdm: momentum %g, weight_decay %g", momentum,
              weight_decay);
  CMX_REQUIRE((buf == nullptr) == (momentum == 0.0), CMX_ERR_ARG,
              "sgdm: the momentum buffer is given exactly when momentum != 0 (momentum %g)", momentum);
  CMX_REQUIRE(!nesterov || momentum > 0.0, CMX_ERR_ARG, "sgdm: nesterov needs momentum > 0");
  CMX_REQUIRE(!shadow || shadow_dtype == 1 || shadow_dtype == 2, CMX_ERR_ARG, "sgdm: shadow dtype %d", shadow_dtype);
  CMX_REQUIRE(p && g && decay64 && lr_ptr, CMX_ERR_ARG, "sgdm: p, g, decay64 and lr_ptr must be given");
  if (n == 0) return CMX_OK;
  // max_blocks > 0 caps the grid (the launch then keeps to that share of the chip)
  long blocks = (n / 4 + 255) / 256;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  // nontemporal p / g / buf traffic (CMX_SGDM_NT=0: cached)
  static int& nt = cmx_knob("SGDM_NT", 1);
  const float mu = (float)momentum, wd = (float)weight_decay;
#define CMX_SGDM_(S_, NT_, MOM_)                                                                                   \
  hipLaunchKernelGGL((sgdm_kernel<S_, NT_, MOM_>), dim3((unsigned)blocks), dim3(256), 0, s, p, g, buf, (S_*)shadow, \
                     decay64, (long)n, lr_ptr, mu, wd, nesterov, grad_scale, loss_scale, found_inf)
#define CMX_SGDM(S_, NT_)                      \
  do {                                          \
    if (buf) CMX_SGDM_(S_, NT_, true);          \
    else CMX_SGDM_(S_, NT_, false);             \
  } while (0)
  if (shadow && shadow_dtype == 2) {
    if (nt) CMX_SGDM(f16, true);
    else CMX_SGDM(f16, false);
  } else {
    if (nt) CMX_SGDM(bf16, true);
    else CMX_SGDM(bf16, false);
  }
#undef CMX_SGDM
#undef CMX_SGDM_
  return cmx_check_launch("sgdm_step");
}

}  // extern "C"
