// fft16.hpp — the radix-16 in-LDS FFT of the tuned complex<float> kernels: packed complex ops, dft16, the LDS pad,
// the device plan (FftDev) and its host table builder (FftPlan). Shared by the FFT filter (fftconv.hip) and the split
// FilterSink / FilterSource stages (fftsplit.hip). Include it after `#pragma clang fp contract(fast)`.
#pragma once
#include "sdrhip_internal.hpp"

#include <cmath>
#include <vector>

namespace {


constexpr int FT = 1024;       // lanes per workgroup
constexpr int MAX_PASS = 16;

struct FftDev {
  int L, npass;
  int radix[MAX_PASS];   // forward pass order (DIF); the inverse walks it backwards
  const float2 *W;       // W[t] = exp(-2 pi i t / L)
  const float2 *T;       // per radix-16 pass q: T[toff[q] + (k-1)*s_q + j] = W^(j tw_q k), k = 1..15 (coalesced along j)
  int toff[MAX_PASS];
};

// Complex arithmetic on register PAIRS: one packed instruction handles (re, im) together, and the op_sel / neg modifiers
// of the packed forms (which 32-bit half of each source feeds the low and the high result, negated or not) fold the
// multiplications by +-i into the add that follows. Written as instructions: left to the compiler's SLP vectoriser the
// same arithmetic came out as 3 packed instructions per complex product (each computing a half that is thrown away) and
// one v_mov_b32 per 4 arithmetic instructions to re-pair halves — 1 924 vector instructions per wave and block of the
// 16384-point filter where the kernel is bound by vector issue (r08's counters: 61 % busy, no other unit above 30 %).
typedef float v2f __attribute__((ext_vector_type(2)));
#define PK2(name_, text_)                                                                                             \
  __device__ __forceinline__ float2 name_(float2 a, float2 b) {                                                        \
    v2f d;                                                                                                             \
    asm(text_ : "=v"(d) : "v"(__builtin_bit_cast(v2f, a)), "v"(__builtin_bit_cast(v2f, b)));                           \
    return __builtin_bit_cast(float2, d);                                                                              \
  }
PK2(cadd, "v_pk_add_f32 %0, %1, %2")
PK2(csub, "v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]")
PK2(cadd_mi, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]")   // a + (-i) b = (a.x + b.y, a.y - b.x)
PK2(cadd_pi, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]")   // a + (+i) b = (a.x - b.y, a.y + b.x)
PK2(pk_mul_xx, "v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]")              // (a.x b.x, a.y b.x)
#undef PK2
// a * b = (a.x b.x - a.y b.y, a.y b.x + a.x b.y) and a * conj(b): a packed multiply and a packed fused multiply-add
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  const float2 t = pk_mul_xx(a, b);
  v2f d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]"
      : "=v"(d) : "v"(__builtin_bit_cast(v2f, a)), "v"(__builtin_bit_cast(v2f, b)), "v"(__builtin_bit_cast(v2f, t)));
  return __builtin_bit_cast(float2, d);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {
  const float2 t = pk_mul_xx(a, b);
  v2f d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]"
      : "=v"(d) : "v"(__builtin_bit_cast(v2f, a)), "v"(__builtin_bit_cast(v2f, b)), "v"(__builtin_bit_cast(v2f, t)));
  return __builtin_bit_cast(float2, d);
}
// the same with a wave-uniform constant factor in a scalar register pair
template <bool CONJ>
__device__ __forceinline__ float2 cmul_k(float2 a, float wr, float wi) {
  const v2f w = {wr, wi};
  v2f t, d;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(t) : "v"(__builtin_bit_cast(v2f, a)), "s"(w));
  if (CONJ) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(d) : "v"(__builtin_bit_cast(v2f, a)), "s"(w), "v"(t));
  else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]" : "=v"(d) : "v"(__builtin_bit_cast(v2f, a)), "s"(w), "v"(t));
  return __builtin_bit_cast(float2, d);
}
__device__ __forceinline__ float2 mul_mi(float2 a) { return cadd_mi(make_float2(0.f, 0.f), a); }   // a * (-i)
__device__ __forceinline__ float2 mul_pi(float2 a) { return cadd_pi(make_float2(0.f, 0.f), a); }   // a * (+i)
// the radix-4 butterfly every pass is made of: (x0..x3) -> (X0..X3), X_m = sum_k x_k exp(SIGN 2 pi i k m / 4); 8 packed adds
template <int SIGN>
__device__ __forceinline__ void bfly4(float2 x0, float2 x1, float2 x2, float2 x3, float2 &X0, float2 &X1, float2 &X2, float2 &X3) {
  const float2 t0 = cadd(x0, x2), t1 = csub(x0, x2), t2 = cadd(x1, x3), d = csub(x1, x3);
  X0 = cadd(t0, t2); X2 = csub(t0, t2);
  if (SIGN < 0) { X1 = cadd_mi(t1, d); X3 = cadd_pi(t1, d); }   // t1 -+ i d
  else { X1 = cadd_pi(t1, d); X3 = cadd_mi(t1, d); }
}

// LDS index of element i: 4 pad elements after every 64, so that the stride-4 radix-16 pass (lanes 64 elements
// = 512 B apart) spreads over the banks instead of hitting one
__device__ __forceinline__ int PAD(int i) { return i + ((i >> 6) << 2); }

// in-place 16-point DFT, v[m] <- sum_k v[k] exp(SIGN 2 pi i k m / 16), as 4 x 4 (k = a + 4b, m = c + 4d)
// LOW_HALF: v[8..15] are zeros and not read (the zero-padded block of FilterSink: step 1 is a 2-point DFT per a)
template <int SIGN, bool LOW_HALF = false>
__device__ __forceinline__ void dft16(float2 *v) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
  // step 1: for each a, the 4-point DFT over b of (v[a], v[a+4], v[a+8], v[a+12]) -> Y_a[c] kept at v[a + 4c]
  if (LOW_HALF) {
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const float2 x0 = v[a], x1 = v[a + 4];
      v[a] = cadd(x0, x1); v[a + 8] = csub(x0, x1);
      v[a + 4] = SIGN < 0 ? cadd_mi(x0, x1) : cadd_pi(x0, x1);
      v[a + 12] = SIGN < 0 ? cadd_pi(x0, x1) : cadd_mi(x0, x1);
    }
  } else {
#pragma unroll
    for (int a = 0; a < 4; a++) bfly4<SIGN>(v[a], v[a + 4], v[a + 8], v[a + 12], v[a], v[a + 4], v[a + 8], v[a + 12]);
  }
  // step 2: Z_a[c] = W16^(a c) Y_a[c]   (W16 = exp(SIGN 2 pi i / 16)); a c in {1,2,3,2,4,6,3,6,9}: the factor is
  // (wr, SIGN wi), i.e. the constant (wr, wi) or its conjugate
  constexpr bool CJ = SIGN < 0;
  v[1 + 4] = cmul_k<CJ>(v[1 + 4], C1, S1);           // a=1,c=1: W^1 = (cos pi/8, SIGN sin pi/8)
  v[1 + 8] = cmul_k<CJ>(v[1 + 8], H, H);             // a=1,c=2: W^2
  v[1 + 12] = cmul_k<CJ>(v[1 + 12], S1, C1);         // a=1,c=3: W^3
  v[2 + 4] = cmul_k<CJ>(v[2 + 4], H, H);             // a=2,c=1: W^2
  v[2 + 8] = SIGN < 0 ? mul_mi(v[2 + 8]) : mul_pi(v[2 + 8]);   // a=2,c=2: W^4 = SIGN i
  v[2 + 12] = cmul_k<CJ>(v[2 + 12], -H, H);          // a=2,c=3: W^6
  v[3 + 4] = cmul_k<CJ>(v[3 + 4], S1, C1);           // a=3,c=1: W^3
  v[3 + 8] = cmul_k<CJ>(v[3 + 8], -H, H);            // a=3,c=2: W^6
  v[3 + 12] = cmul_k<CJ>(v[3 + 12], -C1, -S1);       // a=3,c=3: W^9 = -W^1
  // step 3: for each c, the 4-point DFT over a of Z_a[c] (at v[a + 4c]) -> X[c + 4d]
  float2 o[16];
#pragma unroll
  for (int c = 0; c < 4; c++) bfly4<SIGN>(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3], o[c], o[c + 4], o[c + 8], o[c + 12]);
#pragma unroll
  for (int m = 0; m < 16; m++) v[m] = o[m];
}

// The last two passes of a plan that ends in radix 4 (stride 2) and radix 2 (stride 1) — 2048 = 16 x 16 x 4 x 2 — work
// inside groups of 8 CONSECUTIVE elements: one lane runs both on a group held in registers (same butterflies, same
// twiddles W8^(j m), same element order as the two LDS passes they replace, so the spectrum layout is unchanged).
// forward (decimation in frequency): radix 4 over (e[j], e[j+2], e[j+4], e[j+6]), j = 0, 1, then radix 2 over the pairs
__device__ __forceinline__ void dif8_fwd(float2 *e) {
  constexpr float H = 0.70710678118654752f;
  float2 a0, a1, a2, a3, b0, b1, b2, b3;
  bfly4<-1>(e[0], e[2], e[4], e[6], a0, a1, a2, a3);
  bfly4<-1>(e[1], e[3], e[5], e[7], b0, b1, b2, b3);
  b1 = cmul_k<true>(b1, H, H);      // W8^1 = (H, -H)
  b2 = mul_mi(b2);                  // W8^2 = -i
  b3 = cmul_k<true>(b3, -H, H);     // W8^3 = (-H, -H)
  e[0] = cadd(a0, b0); e[1] = csub(a0, b0); e[2] = cadd(a1, b1); e[3] = csub(a1, b1);
  e[4] = cadd(a2, b2); e[5] = csub(a2, b2); e[6] = cadd(a3, b3); e[7] = csub(a3, b3);
}
// backward (decimation in time): radix 2 over the pairs, then radix 4 with the conjugate twiddles
__device__ __forceinline__ void dit8_inv(float2 *e) {
  constexpr float H = 0.70710678118654752f;
  const float2 a0 = cadd(e[0], e[1]), b0 = csub(e[0], e[1]), a1 = cadd(e[2], e[3]), b1 = csub(e[2], e[3]);
  const float2 a2 = cadd(e[4], e[5]), b2 = csub(e[4], e[5]), a3 = cadd(e[6], e[7]), b3 = csub(e[6], e[7]);
  bfly4<1>(a0, a1, a2, a3, e[0], e[2], e[4], e[6]);
  bfly4<1>(b0, cmul_k<false>(b1, H, H), mul_pi(b2), cmul_k<false>(b3, -H, H), e[1], e[3], e[5], e[7]);
}

// twiddles W^(j tw k), k = 1..15, of radix-16 pass q for butterfly column j: straight from the pass's own table
// (lanes walk consecutive j: 15 coalesced loads that hit L1/L2). Deriving them from 4 table entries with 11 complex
// products cost a quarter of the kernel (ablation: 0.80 -> 0.61 ms).
__device__ __forceinline__ void twiddles16(const FftDev &p, int q, int s, int j, float2 *w) {
  const float2 *t = p.T + p.toff[q] + j;
  if (s >= 4) {   // a pass of stride 4 or more: its table (15 s entries) does not stay in L1 — 2 loads and 13 products (2 packed
                  // instructions each) instead of 15 loads through L2
    const float2 w1 = t[0], w2 = cmul(w1, w1), w4 = t[3 * s], w8 = cmul(w4, w4);
    w[1] = w1; w[2] = w2; w[4] = w4; w[8] = w8;
    w[3] = cmul(w1, w2); w[5] = cmul(w4, w1); w[6] = cmul(w4, w2); w[7] = cmul(w4, w[3]);
    w[9] = cmul(w8, w1); w[10] = cmul(w8, w2); w[11] = cmul(w8, w[3]); w[12] = cmul(w8, w4);
    w[13] = cmul(w8, w[5]); w[14] = cmul(w8, w[6]); w[15] = cmul(w8, w[7]);
    return;
  }
#pragma unroll
  for (int k = 1; k < 16; k++) w[k] = t[(k - 1) * s];
}

// the 15 twiddles of a radix-16 pass from the two seeds w1 = W^(j tw), w4 = W^(4 j tw) the 2-load form reads (already in registers),
// applied as they are made, v[k] *= w^k (CONJ: the conjugates): 8 twiddles live instead of 15 (the pipelined form holds the
// next block's inputs in 32 registers through the passes that use this)
template <bool CONJ>
__device__ __forceinline__ void twiddle_apply_seeded(float2 *v, float2 w1, float2 w4) {
  auto mul = [](float2 x, float2 w) { return CONJ ? cmulc(x, w) : cmul(x, w); };
  const float2 w2 = cmul(w1, w1), w3 = cmul(w1, w2);
  v[1] = mul(v[1], w1); v[2] = mul(v[2], w2); v[3] = mul(v[3], w3); v[4] = mul(v[4], w4);
  const float2 w5 = cmul(w4, w1), w6 = cmul(w4, w2), w7 = cmul(w4, w3), w8 = cmul(w4, w4);
  v[5] = mul(v[5], w5); v[6] = mul(v[6], w6); v[7] = mul(v[7], w7); v[8] = mul(v[8], w8);
  v[9] = mul(v[9], cmul(w8, w1)); v[10] = mul(v[10], cmul(w8, w2)); v[11] = mul(v[11], cmul(w8, w3)); v[12] = mul(v[12], cmul(w8, w4));
  v[13] = mul(v[13], cmul(w8, w5)); v[14] = mul(v[14], cmul(w8, w6)); v[15] = mul(v[15], cmul(w8, w7));
}

// forward, decimation in frequency: natural order in, digit-reversed order out; NT lanes, passes `first` ... npass - 1
// (FilterSink runs pass 0 itself on its zero-padded block)
template <int NT>
__device__ __forceinline__ void dif_passes(float2 *x, const FftDev &p, int tid, int first) {
  int n = p.L;
  for (int q = 0; q < first; q++) n /= p.radix[q];
  for (int pass = first; pass < p.npass; pass++) {
    const int r = p.radix[pass], s = n / r, tw = p.L / n;
    if (r == 16) {
      for (int b = tid; b < p.L / 16; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        float2 v[16], w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = x[PAD(base + k * s)];
        dft16<-1>(v);
        if (s > 1) {
          twiddles16(p, pass, s, j, w);
#pragma unroll
          for (int k = 1; k < 16; k++) v[k] = cmul(v[k], w[k]);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) x[PAD(base + k * s)] = v[k];
      }
    } else if (r == 4) {
      for (int b = tid; b < p.L / 4; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        const float2 a0 = x[PAD(base)], a1 = x[PAD(base + s)], a2 = x[PAD(base + 2 * s)], a3 = x[PAD(base + 3 * s)];
        float2 X0, X1, X2, X3;
        bfly4<-1>(a0, a1, a2, a3, X0, X1, X2, X3);
        x[PAD(base)] = X0;
        x[PAD(base + s)] = cmul(X1, p.W[j * tw]);
        x[PAD(base + 2 * s)] = cmul(X2, p.W[2 * j * tw]);
        x[PAD(base + 3 * s)] = cmul(X3, p.W[3 * j * tw]);
      }
    } else {   // radix 2
      for (int b = tid; b < p.L / 2; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        const float2 a0 = x[PAD(base)], a1 = x[PAD(base + s)];
        x[PAD(base)] = cadd(a0, a1);
        x[PAD(base + s)] = cmul(csub(a0, a1), p.W[j * tw]);
      }
    }
    __syncthreads();
    n = s;
  }
}

// backward (unnormalised), decimation in time: digit-reversed order in, natural order out; NT lanes. SEEDED: the radix-16
// passes of stride >= 4 make their twiddles from the two seeds as they apply them (twiddle_apply_seeded: 8 live instead of
// 15, for callers that hold other values in registers across the passes)
template <int NT, bool SEEDED = false>
__device__ __forceinline__ void dit_passes(float2 *x, const FftDev &p, int tid) {
  int n = 1;
  for (int pass = p.npass - 1; pass >= 0; pass--) {
    const int r = p.radix[pass], s = n;
    n *= r;
    const int tw = p.L / n;
    if (r == 16) {
      for (int b = tid; b < p.L / 16; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        float2 v[16], w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = x[PAD(base + k * s)];
        if (SEEDED && s >= 4) {
          const float2 *t = p.T + p.toff[pass] + j;
          twiddle_apply_seeded<true>(v, t[0], t[3 * s]);
        } else if (s > 1) {
          twiddles16(p, pass, s, j, w);
#pragma unroll
          for (int k = 1; k < 16; k++) v[k] = cmulc(v[k], w[k]);
        }
        dft16<1>(v);
#pragma unroll
        for (int k = 0; k < 16; k++) x[PAD(base + k * s)] = v[k];
      }
    } else if (r == 4) {
      for (int b = tid; b < p.L / 4; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        const float2 a0 = x[PAD(base)];
        const float2 a1 = cmulc(x[PAD(base + s)], p.W[j * tw]);
        const float2 a2 = cmulc(x[PAD(base + 2 * s)], p.W[2 * j * tw]);
        const float2 a3 = cmulc(x[PAD(base + 3 * s)], p.W[3 * j * tw]);
        float2 X0, X1, X2, X3;
        bfly4<1>(a0, a1, a2, a3, X0, X1, X2, X3);
        x[PAD(base)] = X0; x[PAD(base + s)] = X1; x[PAD(base + 2 * s)] = X2; x[PAD(base + 3 * s)] = X3;
      }
    } else {
      for (int b = tid; b < p.L / 2; b += NT) {
        const int j = b & (s - 1), base = (b / s) * n + j;
        const float2 a0 = x[PAD(base)], a1 = cmulc(x[PAD(base + s)], p.W[j * tw]);
        x[PAD(base)] = cadd(a0, a1);
        x[PAD(base + s)] = csub(a0, a1);
      }
    }
    __syncthreads();
  }
}

__device__ void fft_forward_dif(float2 *x, const FftDev &p, int tid) { dif_passes<FT>(x, p, tid, 0); }
__device__ void fft_inverse_dit(float2 *x, const FftDev &p, int tid) { dit_passes<FT>(x, p, tid); }

struct FftPlan {
  int L = 0;
  FftDev dev{};
  DevBuf<float2> W, T;
  DevBuf<int> perm_d;
  std::vector<int> perm;   // position -> frequency index after the forward DIF

  void build(sdrhip_ctx *ctx, int L_) {
    SDRHIP_REQUIRE(L_ >= 4 && L_ <= 16384 && (L_ & (L_ - 1)) == 0, SDRHIP_E_UNSUPPORTED,
                   "FFT size %d: need a power of two in [4,16384]", L_);
    L = L_;
    int lg = 0; while ((1 << lg) < L) lg++;
    dev.L = L; dev.npass = 0;
    // radix-16 passes (one LDS round trip per 4 bits) first, then what is left of log2 L
    int left = lg;
    while (left >= 4) { dev.radix[dev.npass++] = 16; left -= 4; }
    if (left >= 2) { dev.radix[dev.npass++] = 4; left -= 2; }
    if (left) dev.radix[dev.npass++] = 2;
    std::vector<float2> w(L);
    for (int t = 0; t < L; t++) {
      const double ang = -2.0 * M_PI * (double)t / (double)L;
      w[t] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    W.alloc(L); W.upload(w.data(), L, ctx->stream);
    dev.W = W.p;
    {   // per-pass twiddle tables of the radix-16 passes (the last pass, stride 1, has none)
      std::vector<float2> tt;
      int n = L;
      for (int q = 0; q < dev.npass; q++) {
        const int r = dev.radix[q], s = n / r, tw = L / n;
        dev.toff[q] = (int)tt.size();
        if (r == 16 && s > 1)
          for (int k = 1; k < 16; k++)
            for (int j = 0; j < s; j++) {
              const double ang = -2.0 * M_PI * (double)(((long)j * tw * k) % L) / (double)L;
              tt.push_back(make_float2((float)std::cos(ang), (float)std::sin(ang)));
            }
        n = s;
      }
      if (tt.empty()) tt.push_back(make_float2(1.f, 0.f));
      T.alloc(tt.size()); T.upload(tt.data(), tt.size(), ctx->stream);
      dev.T = T.p;
    }
    perm.resize(L);
    for (int pos = 0; pos < L; pos++) {
      int rem = pos, n = L, k = 0, mult = 1;
      for (int ps = 0; ps < dev.npass; ps++) {
        const int r = dev.radix[ps], s = n / r, m = rem / s;
        rem -= m * s; k += m * mult; mult *= r; n = s;
      }
      perm[pos] = k;
    }
    perm_d.alloc(L); perm_d.upload(perm.data(), L, ctx->stream);
  }
  size_t lds_bytes() const { return (size_t)(L + (L >> 6) * 4) * sizeof(float2); }
};

}  // namespace
