// tuner.hip — the tuner bank: C independent IQBaseBand<int16_t> channels (+ fused FM / AM / USB demodulator) over ONE
// shared input row (sdrhip.h, "tuner bank"). Shared by all channels: the input, ONE FIR history, the absolute sample
// index, order, decimation, epilogue, the LUT. Per channel: taps, LUT increment, sign and phase origin, the open window's
// partial sum, the FM angle — and, in a bank made by sdrhip_tunermodes_i16_create, the demodulator. Reference arithmetic as iqbb_common.hpp lists it. A channel of the bank is presented to the
// one-tune plan's device helpers as a one-channel IqbbArgs view (channel_view) with channel index 0, and the host rules
// come from the header the one-tune plan (iqbb_i16.hip) takes them from:
//   iqbb_common.hpp   load_x, rotate / rotate_i16, finalize_group, epilogue_and_roll (and through them box_div; am_i16,
//                     usb_i16, fm_phi: fm_phi.hpp)
//   iqbb_host.hpp     call_geometry, tap_in_range, tap_fits_planes, pack_valu_taps, split_planes, planes_const, hot_row,
//                     reconfigured_ring_row
//
// Two kernels, both bit-exact (each a __device__ body behind its entry points: one instance per demodulator and input kind,
// and tuner_i16_modes_valu_kernel / tuner_i16_modes_mfma_kernel per input kind for a bank with a demodulator per channel):
//   tuner_i16_valu_kernel   v_dot2 FIR at 8 consecutive samples per lane, one workgroup per (time tile, channel): every
//                           valid plan (order 1 ... 513, decimation 1 ... 512, any call length). Still a COPY of
//                           iqbb_i16_kernel<false, false>'s body (iqbb_common.hpp), to be kept equal line for line.
//   tuner_i16_mfma_kernel   the FIR as an int8 GEMM on v_mfma_i32_32x32x32_i8 with CHANNELS as matrix rows:
//                             Y[(channel, comp)][t] = sum_k A[(channel, comp)][k] * U[k][t],   U[k][t] = u[2 (t - KW + 1) + k]
//                           u = the interleaved (re, im) int16 stream of the ONE input, KW = 16 S the padded filter length,
//                           A = the interleaved tap vectors (re: Kr, -Ki ...; im: Ki, Kr ...) of 16 channels = 32 rows.
//                           Products are made exact by byte planes (iqbb_i16.hip): u = 256 uh + ul' + 128, a = 256 ah + al,
//                             S = 65536 sum(ah uh) + 256 sum(ah ul' + al uh) + sum(al ul') + 128 sum(a)   (mod 2^32).
//                           A workgroup stages the two sample planes of its time tile (with the KW - 1 halo) into LDS ONCE
//                           and walks several channel tiles over them; tap fragments are packed per channel tile on the
//                           host (create / set_taps). A lane ends up with (re, im) of 8 channels at one time column:
//                           recombine, >> 14, rotate by the channel's own increment and phase origin, and add into the
//                           (channel, group) box sums in LDS (through a wave-private transpose tile; wrapping int32 adds commute: ds_add_u32). Decimations 4 ... 512,
//                           taps whose high byte plane fits int8, calls of at least HOT_MIN_IN samples.
// A bank of REAL-input channels (sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create: C BaseBand<int16_t> nodes over ONE
// row of real int16 samples, src/baseband.hh:425-460) is the third template argument of both bodies and of channel_view, behind
// entry points of its own (tuner_bb_i16_valu_kernel, tuner_bb_i16_mfma_kernel and their _modes_ forms):
//   plain form              one wrapping 24-bit multiply-add per tap and component on the raw Q16 (Kr, Ki) pair, >> 16
//   matrix form             U[k][t] = u[t - KW + 1 + k] over the real stream, ONE byte per sample and plane, KW = 32 S with
//                           S = ceil(order / 32): half the K steps and half the staged plane bytes of the complex bank; rows
//                           (c, re) = Kr, (c, im) = Ki; a lane's K slice starts at plane byte tc + 16 hh + 32 s, any byte
//                           alignment (v_alignbyte by off & 3); recombined mod 2^32, >> 16. Same conditions as above.
// The windows of D samples from the first sample on (no D + 1 first window) come from call_geometry(.., real = true);
// finalize_group and epilogue_and_roll see in_real through the channel's view.
#include "iqbb_common.hpp"
#include "iqbb_host.hpp"
#include "entry.hpp"

#include <algorithm>
#include <string>

namespace {

constexpr int TUNER_MAX_ORDER = 513, TUNER_MAX_DECIM = 512, TUNER_MAX_CHANNELS = 8192;
constexpr int CT = 16;            // channels per matrix tile (32 rows: re and im of each)
constexpr int TR_STRIDE = 33;    // row stride (int2) of a wave's [channel][column] transpose tile
constexpr int HOT_COLS = 512;     // time columns a hot tile aims at (whole decimation groups)
constexpr int HOT_MIN_D = 4;      // smaller decimations: (channel, group) sums of a tile would not fit LDS
constexpr int HOT_MIN_IN = 512;   // shorter calls hold no tile worth the staging: the plain form
// the EPI template argument of the instances that read the demodulator per channel (TunerArgs::mode); the SDRHIP_EPI_*
// values are 0 ... 3 and the one-tune plan's HOT_EPI_PARTIAL is 4
constexpr int EPI_PER_CHANNEL = -1;

struct TunerArgs {
  IqbbArgs a;               // the call as ONE channel sees it; in / hist: the shared row and ring, taps / acc / fm / out: channel 0's
  const uint32_t *inc;      // per channel: LUT increment
  const int *negative;      // ... sign of the shift
  const uint32_t *phase0;   // ... absolute sample index (low 32 bits) at which the LUT phase counter last restarted
  const int2 *cst;          // ... 128 * sum(a) of the interleaved tap vectors (re, im): the byte-plane constant term
  const int *mode;          // ... SDRHIP_EPI_FM | AM | USB (EPI_PER_CHANNEL instances only; NULL otherwise)
  int C, S, ctiles, ctw;    // channels, K steps of 32 plane bytes, channel tiles, channel tiles walked by one workgroup
  int PLB;                  // bytes of one staged sample plane
};

// Channel c of the bank as the one-tune helpers see a plan's only channel (they are called with channel index 0).
// rolls: this workgroup's channel is the one that rolls the shared history in the call's last tile.
// EPI_PER_CHANNEL: the demodulator is the channel's own — c is uniform over the workgroup wherever a view is made (the plain
// form runs one channel per workgroup, the matrix form finalises channel after channel), so the branches on b.epilogue in
// finalize_group and epilogue_and_roll stay uniform. Such a bank has the FM geometry (ovl = 1, the angle cache behind
// ybuf + CGr): an AM / USB channel leaves the overlap slot's ybuf entry unused (epilogue_and_roll starts at a.ovl), and
// neither writes the angle cache nor fm_new — the host keeps its fm entries at 0 (sdrhip_tunermodes_i16_set_mode).
template <int EPI, bool CU8, bool REAL>
__device__ __forceinline__ IqbbArgs channel_view(const TunerArgs &t, int c, bool rolls) {
  IqbbArgs b = t.a;
  b.in_cu8 = CU8; b.in_real = REAL; b.i8 = 0; b.epilogue = EPI == EPI_PER_CHANNEL ? t.mode[c] : EPI;
  b.taps = t.a.taps + (long)c * t.a.OP;
  b.inc = t.inc[c]; b.negative = t.negative[c];
  b.n0_lo = t.a.n0_lo - t.phase0[c];
  b.acc_old = t.a.acc_old + c; b.acc_new = t.a.acc_new + c;
  b.fm_old = t.a.fm_old + c; b.fm_new = t.a.fm_new + c;
  b.out = reinterpret_cast<char *>(t.a.out) + (long)c * t.a.out_stride * (EPI == SDRHIP_EPI_NONE ? 4 : 2);
  if (!rolls) b.tiles = 0;   // (epilogue_and_roll rolls in tile == tiles - 1)
  return b;
}

// ---- plain form: iqbb_i16_kernel's general decimation path over the shared row, one channel per blockIdx.y -----------
// REAL (a bank of BaseBand<int16_t> channels): the staged dwords are sign-extended real samples, a tap is the raw (Kr, Ki)
// int32 pair and one wrapping 24-bit multiply-add per component replaces the dot2 (iqbb_i16_kernel<.., true>); >> 16.
template <int EPI, bool CU8, bool REAL>
__device__ __forceinline__ void tuner_valu_body(const TunerArgs &t) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int c = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const IqbbArgs a = channel_view<EPI, CU8, REAL>(t, c, c == 0);
  const int XS = TI + a.OP + 8;
  uint32_t *xs = smem;                                  // staged samples, x[tb-(OP-1) ...]
  int2 *lut_s = reinterpret_cast<int2 *>(smem + XS);    // 128 entries
  uint32_t *ybuf = smem + XS + 256;                     // CG packed cs16 results (+ the FM angle cache)
  int2 *vbuf = reinterpret_cast<int2 *>(ybuf + 2 * a.CGr);  // TI rotated samples

  const int q0 = tile * a.OG - a.ovl;    // first group (relative to the call's first group) of this tile
  const int tb = a.base0_rel + q0 * a.D; // call-relative index of the tile's first sample
  const int groups_here = min(a.CG, a.n_groups - q0);

  {
    const int first = tb - (a.OP - 1);
    const int need = min(XS, groups_here * a.D + a.OP + 8);
    for (int i = tid; i < need; i += TPB) xs[i] = load_x(a, 0, first + i);
    if (tid < 128) lut_s[tid] = a.lut[tid];
  }
  __syncthreads();

  if (R * tid < groups_here * a.D) {
    int sre[R], sim[R];
#pragma unroll
    for (int r = 0; r < R; r++) { sre[r] = 0; sim[r] = 0; }
    const uint4 *win = reinterpret_cast<const uint4 *>(xs + R * tid);
    uint32_t w[16];
    {
      const uint4 p0 = win[0], p1 = win[1];
      w[0] = p0.x; w[1] = p0.y; w[2] = p0.z; w[3] = p0.w;
      w[4] = p1.x; w[5] = p1.y; w[6] = p1.z; w[7] = p1.w;
    }
    const uint2 *__restrict__ tp = a.taps;
    for (int i0 = 0; i0 < a.OP; i0 += TAPC) {
      const uint4 p2 = win[i0 / 4 + 2], p3 = win[i0 / 4 + 3];
      w[8] = p2.x; w[9] = p2.y; w[10] = p2.z; w[11] = p2.w;
      w[12] = p3.x; w[13] = p3.y; w[14] = p3.z; w[15] = p3.w;
#pragma unroll
      for (int u = 0; u < TAPC; u++) {
        const uint2 k = tp[i0 + u];   // workgroup-uniform -> scalar loads
#pragma unroll
        for (int r = 0; r < R; r++) {
          if (REAL) {
            sre[r] = (int)((unsigned)__mul24((int)k.x, (int)w[u + r]) + (unsigned)sre[r]);
            sim[r] = (int)((unsigned)__mul24((int)k.y, (int)w[u + r]) + (unsigned)sim[r]);
          } else {
            sre[r] = dot2(w[u + r], k.x, sre[r]);
            sim[r] = dot2(w[u + r], k.y, sim[r]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) w[u] = w[u + 8];
    }
    constexpr int FSH = REAL ? 16 : 14;   // Traits<int16_t>::shift vs the literal 14 of IQBaseBand (src/baseband.hh:459, :235)
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int rel = tb + R * tid + r;
      int2 v = rotate(a, lut_s, make_int2(sre[r] >> FSH, sim[r] >> FSH), a.n0_lo + (uint32_t)rel);
      if (rel < 0 || rel >= a.N) v = make_int2(0, 0);   // outside this call
      vbuf[R * tid + r] = v;
    }
  }
  __syncthreads();

  for (int ql = tid; ql < groups_here; ql += TPB) {
    const int q = q0 + ql;
    if (q < 0) continue;                      // tile 0's overlap slot precedes the call
    int2 s = make_int2(0, 0);
    for (int k = 0; k < a.D; k++) {
      const int2 v = vbuf[ql * a.D + k];
      s.x = (int)((unsigned)s.x + (unsigned)v.x);
      s.y = (int)((unsigned)s.y + (unsigned)v.y);
    }
    finalize_group(a, 0, lut_s, ybuf, ql, q, s, a.D);
  }
  __syncthreads();
  epilogue_and_roll(a, 0, tile, tid, q0, groups_here, ybuf);
}

// ---- hot form -----------------------------------------------------------------------------------------------------------
// LDS: [0, 1024) the rotation table; two sample planes (high bytes, low bytes - 128) of PLB bytes; the channel tile's
// parameters; gsum[CT][CG] box sums; ybuf[CT][2 CGr] results and FM angle cache (finalize_group's layout per channel);
// one [CT][TR_STRIDE] transpose tile per wave.
// Tap fragments (host: pack_tile): v4i index ((ct * S + s) * 2 + plane) * 64 + lane; lane (m = l & 31, hh = l >> 5) holds
// bytes k = 32 s + 16 hh + j of row m, and row m carries the channel and component that hot_row (iqbb_host.hpp) gives:
// by the 32x32 C/D map lane (n, h) then holds, in accumulator registers 2j / 2j + 1, (re, im) of channel 8 h + j of the
// tile at time column n.
// REAL (a bank of BaseBand<int16_t> channels): the element stream is the real sample stream itself, ONE byte per sample and
// plane, so a K step of 32 plane bytes covers 32 samples (KW = 32 S, half the complex bank's K steps for an order), row
// (c, re) is Kr and row (c, im) is Ki, and a lane's K slice starts at plane byte tc + 16 hh + 32 s — any byte alignment.
template <int EPI, bool CU8, bool REAL>
__device__ __forceinline__ void tuner_mfma_body(const TunerArgs &t) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const IqbbArgs &g = t.a;
  const int tile = blockIdx.x, tid = threadIdx.x, l = tid & 63, w = tid >> 6, n = l & 31, h = l >> 5;
  int2 *lut_s = reinterpret_cast<int2 *>(smem);
  unsigned char *plane_h = reinterpret_cast<unsigned char *>(smem + 256);
  unsigned char *plane_l = plane_h + t.PLB;
  uint32_t *cinc = reinterpret_cast<uint32_t *>(plane_l + t.PLB);
  uint32_t *cn0 = cinc + CT;       // (n0 - phase origin) per channel of the tile
  int *cneg = reinterpret_cast<int *>(cn0 + CT);
  int2 *ccst = reinterpret_cast<int2 *>(cneg + CT);
  int2 *gsum = ccst + CT;
  uint32_t *ybuf = reinterpret_cast<uint32_t *>(gsum + CT * g.CG);
  int2 *trbuf = reinterpret_cast<int2 *>(ybuf + CT * 2 * g.CGr);   // 4 waves x [CT][TR_STRIDE]

  const int q0 = tile * g.OG - g.ovl;
  const int tb = g.base0_rel + q0 * g.D;
  const int groups_here = min(g.CG, g.n_groups - q0);
  const int span = groups_here * g.D;          // time columns of this tile
  const int KW = (REAL ? 32 : 16) * t.S;       // padded filter length: plane byte 0 = (re of) sample tb - (KW - 1)

  {   // ---- stage the tile's samples as two byte planes, once for every channel tile ------------------------------------
    IqbbArgs a0 = g; a0.in_cu8 = CU8; a0.in_real = REAL; a0.i8 = 0;
    const int first = tb - (KW - 1), need = REAL ? t.PLB / 4 : t.PLB / 2;
    if (REAL) {   // four samples = one dword of each plane per lane and step
      for (int i = tid; i < need; i += TPB) {
        uint32_t hi = 0, lo = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int k = 4 * i + j;
          const uint32_t x = k < span + KW - 1 ? load_x(a0, 0, first + k) : 0u;
          hi |= ((x >> 8) & 0xffu) << (8 * j);
          lo |= ((x & 0xffu) ^ 0x80u) << (8 * j);
        }
        reinterpret_cast<uint32_t *>(plane_h)[i] = hi;
        reinterpret_cast<uint32_t *>(plane_l)[i] = lo;
      }
    } else
    for (int i = tid; i < need; i += TPB) {
      const uint32_t x = i < span + KW - 1 ? load_x(a0, 0, first + i) : 0u;
      const uint32_t hi = ((x >> 8) & 0xffu) | ((x >> 16) & 0xff00u);
      const uint32_t lo = ((x & 0xffu) | ((x >> 8) & 0xff00u)) ^ 0x8080u;
      reinterpret_cast<uint16_t *>(plane_h)[i] = (uint16_t)hi;
      reinterpret_cast<uint16_t *>(plane_l)[i] = (uint16_t)lo;
    }
    if (tid < 128) lut_s[tid] = g.lut[tid];
  }

  const int nblk = (span + 31) >> 5;
  for (int ci = 0; ci < t.ctw; ci++) {
    const int ct = blockIdx.y * t.ctw + ci;
    if (ct >= t.ctiles) break;
    const int c0 = ct * CT, chans = min(CT, t.C - c0);
    __syncthreads();   // the planes are staged / the previous channel tile's epilogue is through with gsum and ybuf
    for (int i = tid; i < CT * g.CG; i += TPB) gsum[i] = make_int2(0, 0);
    if (tid < CT) {
      const bool live = tid < chans;
      cinc[tid] = live ? t.inc[c0 + tid] : 0u;
      cneg[tid] = live ? t.negative[c0 + tid] : 0;
      cn0[tid] = live ? g.n0_lo - t.phase0[c0 + tid] : 0u;
      ccst[tid] = live ? t.cst[c0 + tid] : make_int2(0, 0);
    }
    __syncthreads();

    // ---- matrix part: wave w takes the column blocks w, w + 4, ... -----------------------------------------------------
    const v4i *frag = g.tapfrag + (size_t)ct * t.S * 2 * 64 + l;
    for (int kb = w; kb < nblk; kb += 4) {
      const int tc = 32 * kb + n;            // the lane's time column within the tile
      v16i acc_hh = {0}, acc_mid = {0}, acc_ll;
#pragma unroll
      for (int r = 0; r < 16; r++) { const int2 k = ccst[8 * h + (r >> 1)]; acc_ll[r] = (r & 1) ? k.y : k.x; }
      const int off = (REAL ? tc : 2 * tc) + 16 * h;   // plane byte of the lane's K slice at step 0 (2-byte aligned; REAL: any alignment)
      const uint32_t *ph = reinterpret_cast<const uint32_t *>(plane_h + (off & ~3));
      const uint32_t *pl = reinterpret_cast<const uint32_t *>(plane_l + (off & ~3));
      const uint32_t sh = (uint32_t)(off & (REAL ? 3 : 2));
      for (int s = 0; s < t.S; s++) {
        const v4i Ah = frag[(2 * s) * 64], Al = frag[(2 * s + 1) * 64];
        uint32_t dh[5], dl[5];
#pragma unroll
        for (int i = 0; i < 5; i++) { dh[i] = ph[8 * s + i]; dl[i] = pl[8 * s + i]; }
        v4i uh, ul;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          uh[i] = (int)__builtin_amdgcn_alignbyte(dh[i + 1], dh[i], sh);
          ul[i] = (int)__builtin_amdgcn_alignbyte(dl[i + 1], dl[i], sh);
        }
        acc_mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al, uh, acc_mid, 0, 0, 0);
        acc_ll = __builtin_amdgcn_mfma_i32_32x32x32_i8(Al, ul, acc_ll, 0, 0, 0);
        acc_hh = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah, uh, acc_hh, 0, 0, 0);
        acc_mid = __builtin_amdgcn_mfma_i32_32x32x32_i8(Ah, ul, acc_mid, 0, 0, 0);
      }
      // ---- recombine, >> 14 (REAL: >> 16), the channel's rotation; then through a wave-private LDS tile [channel][column] so that four
      // lanes per channel each add 8 consecutive columns in registers and touch the (channel, group) box sums once per
      // group they meet (wrapping int32 adds commute: ds_add_u32), not once per column ------------------------------------
      const int rel = tb + tc;               // call-relative sample index
      const bool valid = tc < span && rel >= 0 && rel < g.N;
      int2 *tr = trbuf + w * (CT * TR_STRIDE);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int cl = 8 * h + j;
        const unsigned sr = ((unsigned)acc_hh[2 * j] << 16) + ((unsigned)acc_mid[2 * j] << 8) + (unsigned)acc_ll[2 * j];
        const unsigned si = ((unsigned)acc_hh[2 * j + 1] << 16) + ((unsigned)acc_mid[2 * j + 1] << 8) + (unsigned)acc_ll[2 * j + 1];
        int2 v = make_int2(0, 0);            // outside the call or the tile: r = 0 -> v = 0
        constexpr int FSH = REAL ? 16 : 14;
        if (valid) v = rotate_i16(cinc[cl], cneg[cl], lut_s, make_int2((int)sr >> FSH, (int)si >> FSH), cn0[cl] + (uint32_t)rel);
        tr[cl * TR_STRIDE + n] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      {
        const int cl = l >> 2, cb = 8 * (l & 3);   // lane: channel cl of the tile, columns cb ... cb + 7 of the block
        const int col0 = 32 * kb + cb;
        if (cl < chans && col0 < span) {
          int ql = col0 / g.D, left = g.D - (col0 - ql * g.D);   // the group of the lane's first column, its columns still to come
          int2 s = make_int2(0, 0);
          bool pending = false;
          const int cnt = min(8, span - col0);
          for (int i = 0; i < cnt; i++) {
            const int2 v = tr[cl * TR_STRIDE + cb + i];
            s.x = (int)((unsigned)s.x + (unsigned)v.x); s.y = (int)((unsigned)s.y + (unsigned)v.y);
            pending = true;
            if (--left == 0) {
              atomicAdd(&gsum[cl * g.CG + ql].x, s.x); atomicAdd(&gsum[cl * g.CG + ql].y, s.y);
              s = make_int2(0, 0); pending = false; ql++; left = g.D;
            }
          }
          if (pending) { atomicAdd(&gsum[cl * g.CG + ql].x, s.x); atomicAdd(&gsum[cl * g.CG + ql].y, s.y); }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();   // (the next block rewrites the tile)
    }
    __syncthreads();

    // ---- per channel: carry / first-sample quirk / division / state, then demodulate and store --------------------------
    for (int cl = 0; cl < chans; cl++) {
      const IqbbArgs a = channel_view<EPI, CU8, REAL>(t, c0 + cl, c0 + cl == 0);
      for (int ql = tid; ql < groups_here; ql += TPB) {
        const int q = q0 + ql;
        if (q < 0) continue;
        finalize_group(a, 0, lut_s, ybuf + cl * 2 * g.CGr, ql, q, gsum[cl * g.CG + ql], g.D);
      }
    }
    __syncthreads();
    for (int cl = 0; cl < chans; cl++) {
      const IqbbArgs a = channel_view<EPI, CU8, REAL>(t, c0 + cl, c0 + cl == 0);
      epilogue_and_roll(a, 0, tile, tid, q0, groups_here, ybuf + cl * 2 * g.CGr);
    }
  }
}

// ---- entry points: one instance per (demodulator, input kind) of a single-epilogue bank, and per input kind of a bank with a
// mode per channel. The latter have names of their own: the set of tuner_i16_valu_kernel / tuner_i16_mfma_kernel instances is
// the single-epilogue one.
template <int EPI, bool CU8>
__global__ __launch_bounds__(TPB) void tuner_i16_valu_kernel(const TunerArgs t) { tuner_valu_body<EPI, CU8, false>(t); }
template <int EPI, bool CU8>
__global__ __launch_bounds__(TPB, 2) void tuner_i16_mfma_kernel(const TunerArgs t) { tuner_mfma_body<EPI, CU8, false>(t); }
template <bool CU8>
__global__ __launch_bounds__(TPB) void tuner_i16_modes_valu_kernel(const TunerArgs t) { tuner_valu_body<EPI_PER_CHANNEL, CU8, false>(t); }
template <bool CU8>
__global__ __launch_bounds__(TPB, 2) void tuner_i16_modes_mfma_kernel(const TunerArgs t) { tuner_mfma_body<EPI_PER_CHANNEL, CU8, false>(t); }
// ... and of a bank of real-input channels (sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create): one input kind
template <int EPI>
__global__ __launch_bounds__(TPB) void tuner_bb_i16_valu_kernel(const TunerArgs t) { tuner_valu_body<EPI, false, true>(t); }
template <int EPI>
__global__ __launch_bounds__(TPB, 2) void tuner_bb_i16_mfma_kernel(const TunerArgs t) { tuner_mfma_body<EPI, false, true>(t); }
__global__ __launch_bounds__(TPB) void tuner_bb_i16_modes_valu_kernel(const TunerArgs t) { tuner_valu_body<EPI_PER_CHANNEL, false, true>(t); }
__global__ __launch_bounds__(TPB, 2) void tuner_bb_i16_modes_mfma_kernel(const TunerArgs t) { tuner_mfma_body<EPI_PER_CHANNEL, false, true>(t); }

}  // namespace

struct sdrhip_tuner_i16 {
  sdrhip_ctx *ctx = nullptr;
  int order = 0, OP = 0, S = 0, HH = 0, D = 1, C = 1, epi = 0, in_cu8 = 0, ovl = 0;
  // a bank of BaseBand<int16_t> channels (sdrhip_tunerbb_i16_create): real int16 samples in, raw Q16 taps, S counts K steps
  // of 32 SAMPLES, windows of D samples from the first sample on
  int real = 0;
  // a mode per channel (sdrhip_tunermodes_i16_create): epi = SDRHIP_EPI_FM stands for the bank's geometry, element size and
  // double-buffered angles; the kernels take each channel's demodulator from `mode`
  bool per_channel = false;
  std::vector<int> mode_host;
  DevBuf<int> mode;
  int ctiles = 0;
  size_t max_in = 0, max_out = 0;
  uint64_t n0 = 0;
  int par = 0, par_fm = 0;
  bool force_valu = false;
  int force_ctw = 0;                   // SDRHIP_TUNER_CTW: channel tiles per workgroup of every hot call (0: the launcher's own choice)
  std::vector<int32_t> taps_host;      // C x order x 2
  std::vector<uint32_t> inc_host;
  std::vector<int> neg_host;
  std::vector<char> fits;              // per channel: the taps' high byte plane fits int8
  int misfits = 0;                     // channels whose taps do not (any: the plain form for the whole bank)
  DevBuf<uint2> taps;                  // C x OP x {pack(Kr,-Ki), pack(Ki,Kr)}
  DevBuf<v4i> tapfrag;                 // ctiles x S x 2 x 64
  DevBuf<int2> cst, lut;
  DevBuf<uint32_t> inc, phase0;
  DevBuf<int> negative;
  DevBuf<uint32_t> hist[2];            // ONE ring of HH samples
  DevBuf<int2> acc[2];
  DevBuf<short> fm[2];
  Staging stage;
  std::string last_names;

  Geometry geometry(size_t N) const { return call_geometry(n0, N, D, real != 0); }
  size_t out_elem_bytes() const { return epi == SDRHIP_EPI_NONE ? 4 : 2; }
  size_t in_elem_bytes() const { return (in_cu8 || real) ? 2 : 4; }
  bool hot_plan() const { return !force_valu && misfits == 0 && D >= HOT_MIN_D; }
  bool hot_call(size_t N) const { return hot_plan() && N >= (size_t)HOT_MIN_IN; }
  const char *kernel_name(bool hot) const {
    if (real) return hot ? "tuner_bb_i16_mfma_kernel" : "tuner_bb_i16_valu_kernel";
    return hot ? "tuner_i16_mfma_kernel" : "tuner_i16_valu_kernel";
  }

  // what a call of N >= 1 samples with the geometry g launches (launch and sdrhip_tuner_i16_plan_info)
  struct Plan { bool hot; int CG, OG, tiles, ctw, grid_y, PLB; size_t lds; };
  Plan plan(size_t N, const Geometry &g) const {
    Plan p{};
    p.hot = hot_call(N);
    p.CG = p.hot ? std::max(HOT_COLS / D, ovl ? 4 : 1) : TI / D;   // (FM recomputes one group per tile: at least 3 of 4 are new)
    p.OG = p.CG - ovl;
    const int CGr = (p.CG + 3) & ~3;
    p.tiles = (int)ceil_div((size_t)g.n_groups, (size_t)p.OG);
    if (p.hot) {
      // enough workgroups to fill the device, as many channel tiles per staged sample tile as that leaves
      int ctw = 8; while (ctw > 1 && (size_t)p.tiles * ceil_div((size_t)ctiles, (size_t)ctw) < 1024) ctw >>= 1;
      p.ctw = force_ctw ? force_ctw : ctw;
      const int cols = (p.CG * D + 31) & ~31;
      // (the last K slice of the tile's last column ends at plane byte 2 cols + 32 S; real input: cols + 32 S)
      p.PLB = ((real ? cols + 32 * S : 2 * (cols + 16 * S)) + 16 + 15) & ~15;
      p.grid_y = (int)ceil_div((size_t)ctiles, (size_t)p.ctw);
      p.lds = 1024 + 2 * (size_t)p.PLB + CT * (4 + 4 + 4 + 8) + (size_t)CT * p.CG * 8 + (size_t)CT * 2 * CGr * 4 + 4 * (size_t)CT * TR_STRIDE * 8;
    } else {
      p.grid_y = C;
      p.lds = (TI + (size_t)OP + 8 + 256 + 2 * (size_t)CGr) * 4 + (size_t)TI * 8;
    }
    return p;
  }

  // channel tile ct's fragments (S x 2 x 64 x 16 bytes) and its channels' constant terms (layout: tuner_i16_mfma_kernel)
  void pack_tile(int ct, std::vector<int8_t> &frag, int2 *cst_tile) const {
    // a row of the tap matrix: RL = 32 S elements — KW = 16 S interleaved (re, im) pairs, or KW = 32 S real samples
    const int RL = 32 * S, pad = (real ? RL : RL / 2) - order;
    std::vector<int> are((size_t)CT * RL, 0), aim((size_t)CT * RL, 0);
    for (int cl = 0; cl < CT; cl++) {
      const int c = ct * CT + cl;
      int *re = are.data() + (size_t)cl * RL, *im = aim.data() + (size_t)cl * RL;
      if (c < C && fits[c]) {
        const int32_t *k = taps_host.data() + (size_t)c * order * 2;
        for (int i = 0; i < order; i++) {
          const int kr = k[2 * i], ki = k[2 * i + 1];
          if (real) { re[pad + i] = kr; im[pad + i] = ki; continue; }
          re[2 * (pad + i)] = kr; re[2 * (pad + i) + 1] = -ki;
          im[2 * (pad + i)] = ki; im[2 * (pad + i) + 1] = kr;
        }
      }
      cst_tile[cl] = make_int2(planes_const(re, RL), planes_const(im, RL));
    }
    frag.assign((size_t)S * 2 * 64 * 16, 0);
    for (int st = 0; st < S; st++)
      for (int l = 0; l < 64; l++) {
        const int hh = l >> 5;
        int cl, comp, ah, al;
        hot_row(l & 31, cl, comp);
        const int *row = (comp ? aim.data() : are.data()) + (size_t)cl * RL;
        for (int j = 0; j < 16; j++) {
          split_planes(row[32 * st + 16 * hh + j], ah, al);
          frag[((size_t)(2 * st) * 64 + l) * 16 + j] = (int8_t)ah;
          frag[((size_t)(2 * st + 1) * 64 + l) * 16 + j] = (int8_t)al;
        }
      }
  }
  void upload_tile(int ct) {
    std::vector<int8_t> frag; int2 cst_tile[CT];
    pack_tile(ct, frag, cst_tile);
    const size_t per = (size_t)S * 2 * 64;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(tapfrag.p + (size_t)ct * per, frag.data(), per * sizeof(v4i), hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(cst.p + (size_t)ct * CT, cst_tile, sizeof(cst_tile), hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  }
  void upload_valu(int c) {
    std::vector<uint2> tp(OP);
    pack_valu_taps(taps_host.data() + (size_t)c * order * 2, order, OP, real != 0, tp.data());
    SDRHIP_CHECK_HIP(hipMemcpyAsync(taps.p + (size_t)c * OP, tp.data(), (size_t)OP * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  }

  template <int EPI, bool CU8, bool REAL>
  void launch_kernels(bool hot, const TunerArgs &t, dim3 grid, size_t lds) {
    if constexpr (REAL) {
      if (hot) hipLaunchKernelGGL((tuner_bb_i16_mfma_kernel<EPI>), grid, dim3(TPB), lds, ctx->stream, t);
      else hipLaunchKernelGGL((tuner_bb_i16_valu_kernel<EPI>), grid, dim3(TPB), lds, ctx->stream, t);
    } else {
      if (hot) hipLaunchKernelGGL((tuner_i16_mfma_kernel<EPI, CU8>), grid, dim3(TPB), lds, ctx->stream, t);
      else hipLaunchKernelGGL((tuner_i16_valu_kernel<EPI, CU8>), grid, dim3(TPB), lds, ctx->stream, t);
    }
  }
  template <bool CU8, bool REAL>
  void launch_epi(bool hot, const TunerArgs &t, dim3 grid, size_t lds) {
    if (per_channel) {
      if constexpr (REAL) {
        if (hot) hipLaunchKernelGGL(tuner_bb_i16_modes_mfma_kernel, grid, dim3(TPB), lds, ctx->stream, t);
        else hipLaunchKernelGGL(tuner_bb_i16_modes_valu_kernel, grid, dim3(TPB), lds, ctx->stream, t);
      } else {
        if (hot) hipLaunchKernelGGL((tuner_i16_modes_mfma_kernel<CU8>), grid, dim3(TPB), lds, ctx->stream, t);
        else hipLaunchKernelGGL((tuner_i16_modes_valu_kernel<CU8>), grid, dim3(TPB), lds, ctx->stream, t);
      }
      return;
    }
    switch (epi) {
      case SDRHIP_EPI_FM: launch_kernels<SDRHIP_EPI_FM, CU8, REAL>(hot, t, grid, lds); break;
      case SDRHIP_EPI_AM: launch_kernels<SDRHIP_EPI_AM, CU8, REAL>(hot, t, grid, lds); break;
      case SDRHIP_EPI_USB: launch_kernels<SDRHIP_EPI_USB, CU8, REAL>(hot, t, grid, lds); break;
      default: launch_kernels<SDRHIP_EPI_NONE, CU8, REAL>(hot, t, grid, lds); break;
    }
  }

  void launch(const void *in_dev, size_t N, void *out_dev, size_t out_stride, size_t *n_out) {
    ctx->use();
    if (N == 0) { if (n_out) *n_out = 0; return; }   // empty buffer: nothing moves (src/baseband.hh:200)
    const Geometry g = geometry(N);
    SDRHIP_REQUIRE(out_stride >= (size_t)g.n_out, SDRHIP_E_SIZE, "out_stride %zu < outputs %d", out_stride, g.n_out);
    const Plan p = plan(N, g);
    const bool hot = p.hot;
    TunerArgs t{};
    IqbbArgs &a = t.a;
    a.in = reinterpret_cast<const uint32_t *>(in_dev); a.in_stride = 0; a.in_cu8 = in_cu8; a.in_real = real;
    a.hist_old = hist[par].p; a.hist_new = hist[par ^ 1].p; a.HH = HH;
    a.acc_old = acc[par].p; a.acc_new = acc[par ^ 1].p;
    // (every FM channel writes its fm_new entry in such a call; the other channels of a per-channel bank have 0 in both)
    const bool fm_flip = epi == SDRHIP_EPI_FM && g.n_out >= 2;
    a.fm_old = fm[par_fm].p; a.fm_new = fm[par_fm ^ 1].p;
    a.taps = taps.p; a.lut = lut.p; a.tapfrag = tapfrag.p;
    a.OP = OP; a.D = D; a.N = (int)N; a.n0_lo = (uint32_t)n0;
    a.base0_rel = g.base0_rel; a.n_groups = g.n_groups; a.n_out = g.n_out; a.extra0 = g.extra0;
    a.ovl = ovl;
    a.CG = p.CG; a.OG = p.OG; a.CGr = (a.CG + 3) & ~3;
    a.out = out_dev; a.out_stride = (long)out_stride; a.epilogue = epi;
    a.tiles = p.tiles; a.tpw = 1; a.lpg = 1;
    t.inc = inc.p; t.negative = negative.p; t.phase0 = phase0.p; t.cst = cst.p; t.mode = mode.p;
    t.C = C; t.S = S; t.ctiles = ctiles; t.ctw = p.ctw; t.PLB = p.PLB;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.grid_y);
    const size_t lds = p.lds;
    // (every valid plan fits: the plain form needs at most 44 KB at decimation 1, the matrix form 55200 B at decimation 4 and 513
    // taps; a real-input bank's matrix form 53152 B there: its planes hold one byte per sample)
    SDRHIP_REQUIRE(lds <= 64 * 1024, SDRHIP_E_HIP, "internal error: %zu B of LDS for a valid plan", lds);
    if (real) launch_epi<false, true>(hot, t, grid, lds);
    else if (in_cu8) launch_epi<true, false>(hot, t, grid, lds);
    else launch_epi<false, false>(hot, t, grid, lds);
    SDRHIP_CHECK_HIP(hipGetLastError());
    par ^= 1;
    if (fm_flip) par_fm ^= 1;
    n0 += N;
    last_names = kernel_name(hot);
    if (n_out) *n_out = (size_t)g.n_out;
  }
};

static inline bool valid_mode(int m) { return m == SDRHIP_EPI_FM || m == SDRHIP_EPI_AM || m == SDRHIP_EPI_USB; }

// the argument rules of the four create calls: host only, nothing is allocated before them (all pointers non-NULL)
static void tuner_check_args(const int32_t *taps, int order, const int32_t *lut, const int *modes, int decim, int channels, size_t max_in,
                             int epilogue, bool real) {
  SDRHIP_REQUIRE(order >= 1 && order <= TUNER_MAX_ORDER, SDRHIP_E_UNSUPPORTED, "order %d outside [1,%d]", order, TUNER_MAX_ORDER);
  SDRHIP_REQUIRE(decim >= 1, SDRHIP_E_INVALID, "decim %d < 1", decim);
  SDRHIP_REQUIRE(decim <= TUNER_MAX_DECIM, SDRHIP_E_UNSUPPORTED, "decim %d > %d", decim, TUNER_MAX_DECIM);
  require_channels(channels, TUNER_MAX_CHANNELS);
  require_max_in(max_in);
  SDRHIP_REQUIRE(epilogue >= SDRHIP_EPI_NONE && epilogue <= SDRHIP_EPI_USB, SDRHIP_E_INVALID, "bad epilogue %d", epilogue);
  for (int c = 0; modes && c < channels; c++)
    SDRHIP_REQUIRE(valid_mode(modes[c]), SDRHIP_E_INVALID, "channel %d: mode %d is none of SDRHIP_EPI_FM, _AM, _USB", c, modes[c]);
  for (size_t i = 0; i < (size_t)channels * order * 2; i++)
    SDRHIP_REQUIRE(tap_in_range(taps[i], real), SDRHIP_E_UNSUPPORTED,
                   real ? "channel %zu: tap %zu = %d exceeds 24 bits" : "channel %zu: tap %zu = %d does not fit the packed int16 path",
                   i / ((size_t)order * 2), (i / 2) % (size_t)order, taps[i]);
  for (int i = 0; i < 256; i++)
    SDRHIP_REQUIRE(lut[i] > -(1 << 23) && lut[i] < (1 << 23), SDRHIP_E_UNSUPPORTED, "LUT entry %d = %d exceeds 24 bits", i / 2, lut[i]);
}

// sdrhip_tuner_i16_create (modes = NULL), sdrhip_tunermodes_i16_create (epilogue = SDRHIP_EPI_FM: the geometry) and their
// real-input forms sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create (real)
static void tuner_create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *lut_inc, const int *negative,
                         const int *modes, int decim, int channels, size_t max_in, int epilogue, bool real, sdrhip_tuner_i16 **out) {
  make_handle(ctx, out, taps && lut && lut_inc && negative, [&](sdrhip_tuner_i16 *h) {
    tuner_check_args(taps, order, lut, modes, decim, channels, max_in, epilogue, real);
    h->order = order; h->D = decim; h->C = channels; h->epi = epilogue; h->max_in = max_in; h->real = real ? 1 : 0;
    h->ovl = epilogue == SDRHIP_EPI_FM ? 1 : 0;
    h->OP = (int)ceil_div((size_t)order, (size_t)TAPC) * TAPC;
    h->S = (int)ceil_div((size_t)order, (size_t)(real ? 32 : 16));   // K steps of 32 plane bytes: 16 complex or 32 real samples
    h->HH = (real ? 32 : 16) * h->S;   // >= OP, and the whole ring (reset with keep_history)
    h->ctiles = (int)ceil_div((size_t)channels, (size_t)CT);
    { const char *force = getenv("SDRHIP_TUNER_PATH"); h->force_valu = force && !strcmp(force, "valu"); }
    if (const char *f = getenv("SDRHIP_TUNER_CTW")) { if (f[0] && !f[1] && strchr("1248", f[0])) h->force_ctw = f[0] - '0'; }
    h->taps_host.assign(taps, taps + (size_t)channels * order * 2);
    h->inc_host.assign(lut_inc, lut_inc + channels);
    h->neg_host.resize(channels);
    for (int c = 0; c < channels; c++) h->neg_host[c] = negative[c] ? 1 : 0;
    h->fits.resize(channels);
    for (int c = 0; c < channels; c++) { const int32_t *k = taps + (size_t)c * order * 2; h->fits[c] = std::all_of(k, k + 2 * order, tap_fits_planes); h->misfits += h->fits[c] ? 0 : 1; }
    hipStream_t st = ctx->stream;
    h->taps.alloc((size_t)channels * h->OP);
    {
      std::vector<uint2> all((size_t)channels * h->OP);
      for (int c = 0; c < channels; c++) pack_valu_taps(taps + (size_t)c * order * 2, order, h->OP, real, all.data() + (size_t)c * h->OP);
      h->taps.upload(all.data(), all.size(), st);
    }
    h->tapfrag.alloc((size_t)h->ctiles * h->S * 2 * 64);
    h->cst.alloc((size_t)h->ctiles * CT);
    for (int ct = 0; ct < h->ctiles; ct++) h->upload_tile(ct);
    h->lut.alloc(128); h->lut.upload(reinterpret_cast<const int2 *>(lut), 128, st);
    h->inc.alloc(channels); h->inc.upload(h->inc_host.data(), channels, st);
    h->negative.alloc(channels); h->negative.upload(h->neg_host.data(), channels, st);
    h->phase0.alloc(channels); h->phase0.zero(st);
    if (modes) {
      h->per_channel = true;
      h->mode_host.assign(modes, modes + channels);
      h->mode.alloc(channels); h->mode.upload(h->mode_host.data(), channels, st);
    }
    for (int p = 0; p < 2; p++) {
      h->hist[p].alloc(h->HH); h->hist[p].zero(st);
      h->acc[p].alloc(channels); h->acc[p].zero(st);
      h->fm[p].alloc(channels); h->fm[p].zero(st);
    }
    h->max_out = max_in / decim + 2;
    h->last_names = h->kernel_name(h->hot_call(max_in));
  });
}

// what the receiver bank (rxbank.hip) asks of a tuner bank
namespace sdrhip {
sdrhip_ctx *handle_ctx(const sdrhip_tuner_i16 *h) { return h->ctx; }
int handle_channels(const sdrhip_tuner_i16 *h) { return h->C; }
size_t handle_max_in(const sdrhip_tuner_i16 *h) { return h->max_in; }
int tuner_decim(const sdrhip_tuner_i16 *h) { return h->D; }
int tuner_epilogue(const sdrhip_tuner_i16 *h) { return h->epi; }
size_t tuner_in_elem_bytes(const sdrhip_tuner_i16 *h) { return h->in_elem_bytes(); }
}  // namespace sdrhip

extern "C" {

int sdrhip_tuner_i16_create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *lut_inc,
                            const int *negative, int decim, int channels, size_t max_in, int epilogue, sdrhip_tuner_i16 **out) {
  return guarded([&] { tuner_create(ctx, taps, order, lut, lut_inc, negative, nullptr, decim, channels, max_in, epilogue, false, out); });
}

int sdrhip_tunermodes_i16_create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *lut_inc,
                                 const int *negative, const int *modes, int decim, int channels, size_t max_in,
                                 sdrhip_tuner_i16 **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    require_device_for_null_ctx(ctx);
    SDRHIP_REQUIRE(!ctx || modes, SDRHIP_E_INVALID, "modes is NULL");   // (ctx = NULL on a machine with a device: make_handle's message)
    tuner_create(ctx, taps, order, lut, lut_inc, negative, modes, decim, channels, max_in, SDRHIP_EPI_FM, false, out);
  });
}

// The real-input banks check their arguments BEFORE the context (the rules are host rules: a caller can learn them on a
// machine without a device); a NULL context then is SDRHIP_E_NODEVICE where no device exists, SDRHIP_E_INVALID elsewhere.
int sdrhip_tunerbb_i16_create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *lut_inc,
                              const int *negative, int decim, int channels, size_t max_in, int epilogue, sdrhip_tuner_i16 **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps && lut && lut_inc && negative, SDRHIP_E_INVALID, "NULL argument");
    tuner_check_args(taps, order, lut, nullptr, decim, channels, max_in, epilogue, true);
    require_device_for_null_ctx(ctx);
    tuner_create(ctx, taps, order, lut, lut_inc, negative, nullptr, decim, channels, max_in, epilogue, true, out);
  });
}

int sdrhip_tunermodes_bb_i16_create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *lut_inc,
                                    const int *negative, const int *modes, int decim, int channels, size_t max_in,
                                    sdrhip_tuner_i16 **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps && lut && lut_inc && negative && modes, SDRHIP_E_INVALID, "NULL argument");
    tuner_check_args(taps, order, lut, modes, decim, channels, max_in, SDRHIP_EPI_FM, true);
    require_device_for_null_ctx(ctx);
    tuner_create(ctx, taps, order, lut, lut_inc, negative, modes, decim, channels, max_in, SDRHIP_EPI_FM, true, out);
  });
}

// The demodulator node behind channel `channel`'s baseband is replaced (reference: a new node connected in the old one's
// place; FMDemod::config, src/demod.hh:195-212, starts from _last_value = 0 at :210). Both copies of the channel's angle
// become 0: a new FMDemod's state, and the defined state of a channel that is not FM (launch flips the copies for all).
int sdrhip_tunermodes_i16_set_mode(sdrhip_tuner_i16 *h, int channel, int mode) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(h->per_channel, SDRHIP_E_UNSUPPORTED, "the bank has one demodulator for all channels (sdrhip_tunermodes_i16_create makes one per channel)");
    require_channel_range(h, channel);
    SDRHIP_REQUIRE(valid_mode(mode), SDRHIP_E_INVALID, "mode %d is none of SDRHIP_EPI_FM, _AM, _USB", mode);
    h->ctx->use();
    hipStream_t st = h->ctx->stream;   // stream-ordered after the launches already enqueued
    h->mode_host[channel] = mode;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->mode.p + channel, &h->mode_host[channel], sizeof(int), hipMemcpyHostToDevice, st));
    for (int p = 0; p < 2; p++) SDRHIP_CHECK_HIP(hipMemsetAsync(h->fm[p].p + channel, 0, sizeof(short), st));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
  });
}

int sdrhip_tunermodes_i16_get_modes(sdrhip_tuner_i16 *h, int *modes, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && modes, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(h->per_channel, SDRHIP_E_UNSUPPORTED, "the bank has one demodulator for all channels (sdrhip_tunermodes_i16_create makes one per channel)");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_INVALID, "modes holds %d entries, the bank has %d channels", n, h->C);
    std::copy(h->mode_host.begin(), h->mode_host.end(), modes);
  });
}

int sdrhip_tuner_i16_kernel_names(sdrhip_tuner_i16 *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->last_names.c_str(); });
  });
}

int sdrhip_tuner_i16_plan_info(sdrhip_tuner_i16 *h, size_t n_in, int *info, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && info && n >= 10, SDRHIP_E_INVALID, "info must hold 10 ints");
    SDRHIP_REQUIRE(n_in >= 1 && n_in <= h->max_in, SDRHIP_E_SIZE, "n_in %zu outside [1, max_in %zu]", n_in, h->max_in);
    const sdrhip_tuner_i16::Plan p = h->plan(n_in, h->geometry(n_in));
    info[0] = p.hot ? 1 : 0; info[1] = h->S; info[2] = p.CG; info[3] = p.OG; info[4] = p.tiles; info[5] = h->ctiles;
    info[6] = p.ctw; info[7] = p.grid_y; info[8] = p.PLB; info[9] = (int)p.lds;
  });
}

int sdrhip_tuner_i16_out_count(sdrhip_tuner_i16 *h, size_t n_in, size_t *n_out) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && n_out, SDRHIP_E_INVALID, "NULL argument");
    *n_out = n_in ? (size_t)h->geometry(n_in).n_out : 0;
  });
}

// (one wideband input row: there is no in_stride, and the overlap check takes the input as one row against C output rows)
int sdrhip_tuner_i16_process_dev(sdrhip_tuner_i16 *h, const void *in_dev, size_t n_in, void *out_dev, size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_tuner_i16_process_dev");
    if (!call_begin(h, "n_in", n_in, in_dev, out_dev)) { if (n_out) *n_out = 0; return; }
    const size_t no = (size_t)h->geometry(n_in).n_out;
    const Strides s = call_strides("n_in", n_in, 0, no, out_stride, 0);   // (out_stride: launch checks it, after the overlap)
    require_disjoint(in_dev, n_in, n_in, h->in_elem_bytes(), out_dev, s.out, no, h->out_elem_bytes(), 1, (size_t)h->C);
    h->launch(in_dev, n_in, out_dev, s.out, n_out);
  });
}

int sdrhip_tuner_i16_process(sdrhip_tuner_i16 *h, const void *in_host, size_t n_in, void *out_host, size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_tuner_i16_process");
    if (!call_begin(h, "n_in", n_in, in_host, out_host)) { if (n_out) *n_out = 0; return; }
    const Strides s = call_strides("n_in", n_in, 0, (size_t)h->geometry(n_in).n_out, out_stride, STRIDE_OUT);
    // (the output rows are staged at max_out 4-byte slots whatever the element: a demodulated row uses half of its pitch)
    const size_t ib = h->in_elem_bytes(), eb = h->out_elem_bytes(), C = (size_t)h->C;
    size_t produced = 0;
    run_staged(h->ctx, h->stage, h->max_in * 4, C * h->max_out * 4, {in_host, n_in * ib, n_in * ib, 1},
               {out_host, s.out * eb, h->max_out * 4, C}, [&](void *in, void *out) {
                 h->launch(in, n_in, out, h->max_out * 4 / eb, &produced);
                 return produced * eb;
               });
    if (n_out) *n_out = produced;
  });
}

int sdrhip_tuner_i16_set_taps(sdrhip_tuner_i16 *h, int channel, const int32_t *taps) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && taps, SDRHIP_E_INVALID, "NULL argument");
    require_channel_range(h, channel);
    for (int i = 0; i < 2 * h->order; i++)
      SDRHIP_REQUIRE(tap_in_range(taps[i], h->real != 0), SDRHIP_E_UNSUPPORTED,
                     h->real ? "tap %d = %d exceeds 24 bits" : "tap %d = %d does not fit the packed int16 path", i / 2, taps[i]);
    h->ctx->use();
    std::copy(taps, taps + (size_t)h->order * 2, h->taps_host.begin() + (size_t)channel * h->order * 2);
    // (taps whose high byte plane does not fit int8 move the whole bank to the plain form until they are replaced)
    const bool fit = std::all_of(taps, taps + 2 * h->order, tap_fits_planes);
    h->misfits += (h->fits[channel] ? 0 : -1) + (fit ? 0 : 1);
    h->fits[channel] = fit;
    h->upload_valu(channel);   // stream-ordered after the launches already enqueued
    h->upload_tile(channel / CT);
    if (h->n0 == 0) h->last_names = h->kernel_name(h->hot_call(h->max_in));
  });
}

int sdrhip_tuner_i16_set_shift(sdrhip_tuner_i16 *h, int channel, uint32_t lut_inc, int negative) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    hipStream_t st = h->ctx->stream;
    h->inc_host[channel] = lut_inc; h->neg_host[channel] = negative ? 1 : 0;
    const uint32_t p0 = (uint32_t)h->n0;   // _lut_count = 0 (src/freqshift.hh:86): the phase is a closed form of (n - origin)
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->inc.p + channel, &h->inc_host[channel], 4, hipMemcpyHostToDevice, st));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->negative.p + channel, &h->neg_host[channel], 4, hipMemcpyHostToDevice, st));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->phase0.p + channel, &p0, 4, hipMemcpyHostToDevice, st));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
  });
}

int sdrhip_tuner_i16_set_input_format(sdrhip_tuner_i16 *h, int format) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(format == SDRHIP_IN_CS16 || format == SDRHIP_IN_CU8, SDRHIP_E_INVALID, "bad input format %d", format);
    SDRHIP_REQUIRE(!h->real, SDRHIP_E_UNSUPPORTED, "a bank of real-input channels takes real int16 samples only");
    SDRHIP_REQUIRE(h->n0 == 0, SDRHIP_E_INVALID, "the input format can only change before the first buffer / after a reset");
    h->in_cu8 = format == SDRHIP_IN_CU8;
  });
}

int sdrhip_tuner_i16_reset(sdrhip_tuner_i16 *h, int keep_history) {
  return guarded([&] {
    use_handle(h);
    hipStream_t st = h->ctx->stream;
    // bit 0: the FIR ring survives, read ROTATED afterwards (reconfigured_ring_row, iqbb_host.hpp); bit 1: so do the fused
    // FMDemod's last angles (sdrhip_iqbb_i16_reset)
    const bool keep_fm = (keep_history & 2) != 0;
    keep_history &= 1;
    for (int p = 0; p < 2; p++) { h->acc[p].zero(st); if (!keep_fm) h->fm[p].zero(st); }
    const int P = (int)(h->n0 % (uint64_t)h->order);   // the reference's _ring_offset
    if (!keep_history) {
      for (int p = 0; p < 2; p++) h->hist[p].zero(st);
    } else if (P != 0) {
      const int HH = h->HH;
      std::vector<uint32_t> old(HH), neu(HH, 0u);
      SDRHIP_CHECK_HIP(hipMemcpyAsync(old.data(), h->hist[h->par].p, (size_t)HH * 4, hipMemcpyDeviceToHost, st));
      SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
      reconfigured_ring_row(old.data(), HH, h->order, P, neu.data(), HH);
      SDRHIP_CHECK_HIP(hipMemcpyAsync(h->hist[h->par].p, neu.data(), (size_t)HH * 4, hipMemcpyHostToDevice, st));
      SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
    }
    h->phase0.zero(st);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
    h->n0 = 0;
  });
}

int sdrhip_tuner_i16_destroy(sdrhip_tuner_i16 *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
