// iqbb_host.hpp — host-side rules of IQBaseBand<int16_t> that every plan kind must apply alike to stay bit-exact: the
// one-tune plan (iqbb_i16.hip) and the tuner bank (tuner.hip) both take them from here. Plain host functions, no HIP
// runtime calls.
#pragma once
#include "sdrhip_internal.hpp"

namespace sdrhip {

// The decimation groups a call of N >= 1 samples from absolute index n0 on touches: how many, how many of them complete
// in the call (always the first n_out), the call-relative index of the first group's first sample, and whether the
// stream's sample 0 joins group 0. IQBaseBand closes its first window after D + 1 samples (src/baseband.hh:200,212);
// the real-input BaseBand after D (:431-438).
struct Geometry { int n_groups, n_out, base0_rel, extra0; };
inline Geometry call_geometry(uint64_t n0, size_t N, int D, bool real) {
  Geometry g{};
  const uint64_t D64 = (uint64_t)D, shift1 = (D > 1 && !real) ? 1 : 0;
  auto group_of = [&](uint64_t n) -> uint64_t { return n < shift1 ? 0 : (n - shift1) / D64; };
  const uint64_t gf = group_of(n0), gl = group_of(n0 + N - 1);
  const uint64_t last_end = (gl + 1) * D64 - 1 + shift1;
  g.n_groups = (int)(gl - gf + 1);
  g.n_out = g.n_groups - (last_end <= n0 + N - 1 ? 0 : 1);
  g.base0_rel = (int)((int64_t)(gf * D64 + shift1) - (int64_t)n0);
  g.extra0 = (n0 == 0 && shift1) ? 1 : 0;
  return g;
}

// A tap value fits the plan's sample type: int16 beside complex input (-32768 excluded: its negation is packed too),
// 24 bits beside real input.
inline bool tap_in_range(int v, bool real) { return real ? v > -(1 << 23) && v < (1 << 23) : v >= -32767 && v <= 32767; }

// The matrix formulations' byte planes: v = 256 ah + al with al in [-128, 127]. A tap fits them when the high bytes of
// the value and of its negation (both are packed: Kr, -Ki / Ki, Kr) fit int8.
inline void split_planes(int v, int &ah, int &al) { al = ((v + 128) & 255) - 128; ah = (v - al) >> 8; }
inline bool tap_fits_planes(int v) {
  int hp, hn, lo;
  split_planes(v, hp, lo); split_planes(-v, hn, lo);
  return hp <= 127 && hn <= 127;
}
// ... and their constant term 128 * sum(a) over a row of the tap matrix (mod 2^32)
inline int planes_const(const int *a, size_t n) {
  unsigned s = 0;
  for (size_t i = 0; i < n; i++) s += (unsigned)a[i];
  return (int)(128u * s);
}

// Row m of a 32-row tap matrix whose products the 32x32 C/D map hands out so that a lane holds 8 consecutive t: lane
// half hC = (m >> 2) & 1 gets the rows m with register r = (m & 3) + 4 (m >> 3); row m carries t = 8 hC + (r >> 1)
// (one-tune plan: sample of the block; bank: channel of the tile) and component r & 1.
inline void hot_row(int m, int &t, int &comp) {
  const int hC = (m >> 2) & 1, r = (m & 3) + 4 * (m >> 3);
  t = 8 * hC + (r >> 1); comp = r & 1;
}

// The VALU kernel's taps, OP x {pack(Kr, -Ki), pack(Ki, Kr)} (real input: the raw (Kr, Ki) pair), zero-padded at the
// FRONT (older samples) so that the newest sample still meets K[order - 1].
inline void pack_valu_taps(const int32_t *taps, int order, int OP, bool real, uint2 *dst) {
  const int pad = OP - order;
  for (int i = 0; i < pad; i++) dst[i] = make_uint2(0, 0);
  for (int i = 0; i < order; i++) {
    const int kr = taps[2 * i], ki = taps[2 * i + 1];
    if (real) { dst[pad + i] = make_uint2((uint32_t)kr, (uint32_t)ki); continue; }
    dst[pad + i].x = ((uint32_t)(uint16_t)(int16_t)kr) | ((uint32_t)(uint16_t)(int16_t)(-ki) << 16);
    dst[pad + i].y = ((uint32_t)(uint16_t)(int16_t)ki) | ((uint32_t)(uint16_t)(int16_t)kr << 16);
  }
}

// What IQBaseBand::_reconfigure leaves of the FIR ring (src/baseband.hh:175-177: _ring_offset = 0, the ring's contents
// stay where they lie), as one history row (oldest first, the newest at the end) of a plan that starts counting at
// zero: with P = (samples so far) mod order the node afterwards reads the old ring ROTATED — the apparent history,
// oldest first, is ring[1 .. order-1], ring[i] = t[order-P+i] (i < P) or t[i-P] (i >= P), t = the last `order` samples
// in time order (the tail of the source row of HH_src entries). Writes the last order - 1 of new_row's HH_dst entries.
inline void reconfigured_ring_row(const uint32_t *old_row, int HH_src, int order, int P, uint32_t *new_row, int HH_dst) {
  const uint32_t *t = old_row + (HH_src - order);
  uint32_t *d = new_row + (HH_dst - (order - 1));
  for (int k = 0; k + 1 < order; k++) { const int i = k + 1; d[k] = i < P ? t[order - P + i] : t[i - P]; }
}

}  // namespace sdrhip
