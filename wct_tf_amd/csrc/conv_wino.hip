// Reduced-FLOP 3x3 convolution for the wide layers of the stylize path (gfx950 / CDNA4): Winograd F(2,3) along y, direct along x.
//
// Replaces, like conv.hip, what the reference hands to cuDNN through Keras -- pad_reflect + Conv2D 3x3 'valid' + bias + ReLU
// (ops.py:12-19, vgg_normalised.py:28-40, model.py:291), with the x2 nearest upsample in the loader (model.py:293) and the
// 'same' 2x2 max-pool in the epilogue (vgg_normalised.py:42) -- and cuDNN's algorithm selection for 3x3 / stride 1 includes
// Winograd.  Two output rows (2r, 2r+1) of a column take 4 transformed input rows instead of 2 x 3:
//     T0 = d0 - d2   T1 = d1 + d2   T2 = d2 - d1   T3 = d1 - d3          (d_i = padded input row 2r + i, per pixel and channel)
//     U_f[kx] = sum_ky G[f][ky] g[ky][kx],  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]     (per kx, cin, cout; packed at upload)
//     M_f = sum_{kx, cin} U_f[kx] T_f[x + kx]                                                (the MFMA work: 12 products per 2 outputs
//     y(2r) = M0 + M1 + M2      y(2r+1) = M1 - M2 - M3                                        instead of 18: 1.5 x fewer MFMAs)
// The 2-D form F(2x2,3x3) would save 2.25 x but needs 16 fp32 accumulators per 4 outputs: 64 K accumulators per CU bound a
// workgroup to 64 tiles x 64 channels, whose operands (weights 32 KB + patch 10 KB per 16 input channels and 512 MFMA cycles) ask
// the L2 for ~83 B/clk/CU -- more than a CU can take.  The 1-D form keeps 2 accumulators per output: the block is the 256 pixels
// x 128 channels of the direct kernel, ONE block per CU with its 256 accumulator registers in AGPRs.
//
// Error side, measured before anything was built (tools/probe/winograd_error.py, profiles/r06_winograd_error.txt): T is rounded
// to fp16 once more than the direct path's operands; per layer 3.0e-4 .. 6.0e-4 of the output against 2.0e-4 .. 4.0e-4 direct.
//
// Layout in LDS: the transformed patch of a K-chunk (32 input channels), rows (pair-row, f) x 18 pixels (pitch 20) x 64 B with
// the XOR swizzle of conv.hip, double-buffered; the loader takes the four raw rows of a (pair-row, pixel, 16-byte piece) item
// straight from global memory into registers, transforms them with packed fp16 adds and stores four pieces.  MFMA operands as in
// conv.hip: A = weights, pre-packed fragments [Cout/32][f*3+kx][Cin/16][lane][8] streamed from global memory (L2) two taps ahead;
// B = pixels, one ds_read_b128 per fragment a tap ahead; a wave owns MT pixel tiles (2 pair-rows x 16 columns) x NT channel tiles
// x 4 row frequencies.  One LDS-only barrier per K-chunk (s_waitcnt lgkmcnt(0) + s_barrier: the weight loads stay in flight).
//
// Two kernels.  conv3x3_wino_walk_kernel<16,128,1,4>: one block per CU (256 accumulator registers per lane in AGPRs, one wave per
// SIMD), the interleaved schedule, and a block WALKS a static list of tiles -- g, g + grid, .. of the linear order -- with the next
// tile's first patch and weights staged under the current tile's last chunk and epilogue; LDS = two patch buffers (80 KB) + the
// dump area of the idle loader lanes (8 KB) + the layer's bias (4 Cout bytes).  conv3x3_wino_kernel<8,..>: the 8-row shapes for
// grids that do not fill the chip, one tile per block, two blocks per CU.  Both accumulate every output in the same order.
// What the two share is written once, above them: the tile geometry and LDS layout (WinoShape, which also sizes the launchers'
// dynamic LDS), the input transform (wino_T), the loader's and the fragments' addressing (wino_row_offsets .. wino_init_acc) and
// the epilogue (wino_epilogue).  What stays apart is the two kernels themselves -- their schedules, and how much may live in
// registers around the chunk loop, differ ("A block walks its tiles") -- and the body of the interleaved loop, whose
// instruction order is the schedule.
#include "common.h"
#include "conv_tile.h"          // TW, PITCH, BK, u32x4, h2, reflect_idx: shared with conv.hip

namespace {
// The geometry of a tile shape: TH rows x 16 columns of pixels x BN output channels on WM x WN waves.
template <int TH, int BN, int WM, int WN>
struct WinoShape {
  static constexpr int PR = TH / 2;                 // pair-rows of the tile
  static constexpr int MT = (PR / 2) / WM;          // MFMA pixel tiles (2 pair-rows x 16 columns) per wave
  static constexpr int NT = (BN / 32) / WN;
  static constexpr int G = 256 / PR;                // loader threads per pair-row
  static constexpr int SL = (72 + G - 1) / G;       // (pixel, piece) slots per loader thread: 18 x 4 per pair-row
  static constexpr int PATCH_BYTES = PR * 4 * PITCH * 64;
  static_assert(PR % 2 == 0 && (PR / 2) % WM == 0 && 256 % PR == 0 && WM * WN == 4, "tile shape");
  // LDS: the two patch buffers; behind them, in the walking kernel only:
  static constexpr int DUMP_OFF = 2 * PATCH_BYTES;  // where the idle lanes of the last loader slot put their four pieces (8 KB)
  static constexpr int BIAS_OFF = DUMP_OFF + 8192;  // the layer's bias, 4 * Cout bytes
  static size_t patch_lds_bytes() { return 2 * (size_t)PATCH_BYTES; }
  static size_t lds_bytes(int cout) { return BIAS_OFF + 4 * (size_t)cout; }
};

// a - b on eight packed fp16 values: v_pk_add_f16 with the neg modifiers on the second operand (hipcc expands the vector
// subtraction into v_sub_f16 + v_sub_f16_sdwa + v_pack_b32_f16 per pair: three instructions for one)
__device__ __forceinline__ half8 pk_sub(half8 a, half8 b) {
  u32x4 ua = __builtin_bit_cast(u32x4, a), ub = __builtin_bit_cast(u32x4, b), r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned o;
    asm("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(o) : "v"(ua[i]), "v"(ub[i]));
    r[i] = o;
  }
  return __builtin_bit_cast(half8, r);
}

// Row f of T = B^T d on packed fp16 pairs, from the four raw rows d0..d3 of a (pixel, piece) slot.  f is a constant wherever this
// is called, and a literal where a slot's four rows are parked at once: under a loop over f the walking kernel's prologue was
// scheduled differently
__device__ __forceinline__ half8 wino_T(const u32x4 (&raw)[4], int f) {
  const half8 d0 = __builtin_bit_cast(half8, raw[0]), d1 = __builtin_bit_cast(half8, raw[1]);
  const half8 d2 = __builtin_bit_cast(half8, raw[2]), d3 = __builtin_bit_cast(half8, raw[3]);
  return f == 0 ? pk_sub(d0, d2) : f == 1 ? d1 + d2 : f == 2 ? pk_sub(d2, d1) : pk_sub(d1, d3);
}

// ---- the loader's addressing: thread (lpr, ls) takes the slots ls, ls + G, .. of pair-row lpr; slot = pixel * 4 + piece, 72 of them.
// the byte offsets of the four raw rows of pair-row lpr of the tile at row y0
__device__ __forceinline__ void wino_row_offsets(ConvArgs p, int Win, int y0, int lpr, unsigned (&row_off)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int iy = reflect_idx(y0 + 2 * lpr - 1 + i, p.H);
    if (p.upsample) iy >>= 1;
    row_off[i] = (unsigned)(iy * Win) * p.Cin * 2;
  }
}
__device__ __forceinline__ int wino_slot_px(int slot) { return slot < 72 ? slot >> 2 : 0; }
// the byte offset of a slot's column and piece within a raw row of the tile at column x0
__device__ __forceinline__ unsigned wino_col_offset(ConvArgs p, int x0, int slot) {
  int ix = reflect_idx(x0 - 1 + wino_slot_px(slot), p.W);
  if (p.upsample) ix >>= 1;
  return (unsigned)(ix * p.Cin + (slot & 3) * 8) * 2;
}
// where a slot's frequency-0 piece goes in a patch buffer, with the XOR swizzle of conv.hip
__device__ __forceinline__ unsigned wino_slot_dst(int lpr, int slot) {
  const int px = wino_slot_px(slot), piece = slot & 3;
  return ((lpr * 4 * PITCH + px) * 4 + (piece ^ ((px >> 2) & 3))) * 16;
}

// ---- fragment addressing: lane = (column frag_px, pair-row frag_pr, k-group kgrp) of an MFMA pixel tile
// pixel (pair-row wm*MT*2 + frag_pr, column frag_px + kx), k-step ks; (mt, f) rows are immediates
template <int MT>
__device__ __forceinline__ void wino_rd_base(int (&rd_base)[3][2], int wm, int frag_px, int frag_pr, int kgrp) {
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int px = frag_px + kx;
      rd_base[kx][ks] = (((wm * MT * 2 + frag_pr) * 4) * PITCH + px) * 64 + (((ks * 2 + kgrp) ^ ((px >> 2) & 3)) * 16);
    }
}
// the pixel fragment (f, kx, k-step ks) of the wave's pixel tile mt, from the patch buffer at `patch`
__device__ __forceinline__ half8 wino_pixel_frag(const unsigned char* patch, const int (&rd_base)[3][2], int f, int kx, int ks, int mt) {
  return *reinterpret_cast<const half8*>(patch + rd_base[kx][ks] + (mt * 8 + f) * PITCH * 64);
}
template <int MT>
__device__ __forceinline__ void wino_read_b(half8 (&dst)[2][MT], const unsigned char* patch, const int (&rd_base)[3][2], int f, int kx) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) dst[ks][mt] = wino_pixel_frag(patch, rd_base, f, kx, ks, mt);
}
// the lane's share of the address of the weight fragments of the wave's channel tiles; ctile0: the block's first 32-channel tile,
// or 0 where it rides in the scalar offset instead
template <int NT>
__device__ __forceinline__ void wino_wfrag(unsigned (&wfrag)[NT], int ctile0, int wn, int c16, int lane) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wfrag[nt] = ((ctile0 + wn * NT + nt) * 12 * c16 * 512 + lane * 8) * 2;
}
// the scalar share: tap tap12 = f * 3 + kx of K-chunk `chunk`, plus the channel tile's offset wt where wfrag does not hold it
__device__ __forceinline__ int wino_w_soff(int c16, int tap12, int chunk, unsigned wt) { return (tap12 * c16 + chunk * 2) * 1024 + wt; }
__device__ __forceinline__ half8 wino_weight_frag(__amdgpu_buffer_rsrc_t w_rsrc, unsigned wfrag, int ks, int soff) {
  return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, wfrag + ks * 1024, soff, 0));
}
template <int NT>
__device__ __forceinline__ void wino_load_w(half8 (&dst)[NT][2], __amdgpu_buffer_rsrc_t w_rsrc, const unsigned (&wfrag)[NT], int soff) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) dst[nt][ks] = wino_weight_frag(w_rsrc, wfrag[nt], ks, soff);
}

// the bias rides in M1, the one frequency that enters both output rows with +1 (y(2r) = M0 + M1 + M2, y(2r+1) = M1 - M2 - M3):
// acc register r of a tile holds channel (r & 3) + 8 (r >> 2) + 4 kgrp, so bv[nt][rq] = the bias of the four channels from
// 32 nt + 8 rq + 4 kgrp of the wave's first (the 8-row kernels read it from global memory, the walking kernel from its copy in LDS)
template <int MT, int NT>
__device__ __forceinline__ void wino_init_acc(f32x16 (&acc)[4][NT][MT], const f32x4 (&bv)[NT][4]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[f][nt][mt][r] = f == 1 ? bv[nt][r >> 2][r & 3] : 0.f;
}

// ---- epilogue: y(2r) = M0 + M1 + M2, y(2r+1) = M1 - M2 - M3 (the bias came in with M1), ReLU on the rounded pairs, (2x2 max-pool), stores.
// acc register r of a tile holds channel (r & 3) + 8 (r >> 2) + 4 kgrp of pixel (pair-row frag_pr, column frag_px).  The lane's
// coordinates and the relu flag come from the caller: the walking kernel has to make them where it calls (see there).  ConvArgs by
// value: by reference <8,64,2,2> gets two more exec-mask blocks (profiles/wino_shared_isa.txt has the form that was kept).
template <int MT, int NT>
__device__ __forceinline__ void wino_epilogue(ConvArgs p, f32x16 (&acc)[4][NT][MT], int b, int y0, int x0, int n0, int wm, int wn,
                                              int frag_px, int frag_pr, int kgrp, int relu) {
  constexpr int OOB = (int)0x80000000u;
  const int Ho = p.pool ? (p.H + 1) / 2 : p.H, Wo = p.pool ? (p.W + 1) / 2 : p.W;
  const unsigned img_elems = (unsigned)Ho * Wo * p.Cout;
  const __amdgpu_buffer_rsrc_t r16 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y16 + (size_t)b * img_elems), 0, img_elems * 2, 0x00020000);
  const float lo1 = relu ? 0.f : -__builtin_inff();
  const h2 lo2 = {(half_t)lo1, (half_t)lo1};
  const h2 zero2 = {(half_t)0.f, (half_t)0.f};
  const int ox = x0 + frag_px;
  const int chan = n0 + wn * NT * 32;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int oy = y0 + ((wm * MT + mt) * 2 + frag_pr) * 2;        // the even row of this lane's pair
    const bool in0 = (oy < p.H) & (ox < p.W), in1 = (oy + 1 < p.H) & (ox < p.W);
    int off[2];
    if (p.pool) {
      off[0] = in0 && (frag_px & 1) == 0 ? (((oy >> 1) * Wo + (ox >> 1)) * p.Cout + chan + 8 * kgrp) * 2 : OOB;
      off[1] = OOB;
    } else {
      off[0] = in0 ? ((oy * p.W + ox) * p.Cout + chan + 8 * kgrp) * 2 : OOB;
      off[1] = in1 ? (((oy + 1) * p.W + ox) * p.Cout + chan + 8 * kgrp) * 2 : OOB;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      unsigned pk[2][4][2];
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        f32x4 e, o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rq * 4 + j;
          const float m0 = acc[0][nt][mt][r], m1 = acc[1][nt][mt][r], m2 = acc[2][nt][mt][r], m3 = acc[3][nt][mt][r];
          e[j] = (m0 + m1) + m2;
          o[j] = (m1 - m2) - m3;
        }
        h2 e0 = {(half_t)e[0], (half_t)e[1]}, e1 = {(half_t)e[2], (half_t)e[3]};
        h2 o0 = {(half_t)o[0], (half_t)o[1]}, o1 = {(half_t)o[2], (half_t)o[3]};
        e0 = __builtin_elementwise_max(e0, lo2); e1 = __builtin_elementwise_max(e1, lo2);
        o0 = __builtin_elementwise_max(o0, lo2); o1 = __builtin_elementwise_max(o1, lo2);
        if (p.pool) {
          // the row pair is this lane's own (e, o); the column pair sits in lane ^ 1 (DPP quad_perm(1,0,3,2)); cells outside
          // the image are 0, neutral after the ReLU (ceil-mode edge)
          h2 q[2] = {__builtin_elementwise_max(in0 ? e0 : zero2, in1 ? o0 : zero2), __builtin_elementwise_max(in0 ? e1 : zero2, in1 ? o1 : zero2)};
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const unsigned tq = __builtin_bit_cast(unsigned, q[d]);
            const h2 nb = __builtin_bit_cast(h2, __builtin_amdgcn_update_dpp(0, (int)tq, 0xB1, 0xF, 0xF, true));
            q[d] = __builtin_elementwise_max(q[d], nb);
          }
          e0 = q[0]; e1 = q[1];
        }
        pk[0][rq][0] = __builtin_bit_cast(unsigned, e0); pk[0][rq][1] = __builtin_bit_cast(unsigned, e1);
        pk[1][rq][0] = __builtin_bit_cast(unsigned, o0); pk[1][rq][1] = __builtin_bit_cast(unsigned, o1);
      }
      // the two half-waves own interleaved 8-byte pieces: one v_permlane32_swap per dword pairs quad 2m with quad 2m+1 so that
      // the lower half stores channels 16m..16m+7 and the upper half 16m+8..16m+15 -- 16-byte stores (conv.hip's epilogue)
#pragma unroll
      for (int par = 0; par < 2; ++par) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          auto sx = __builtin_amdgcn_permlane32_swap(pk[par][2 * m][0], pk[par][2 * m + 1][0], false, false);
          auto sy = __builtin_amdgcn_permlane32_swap(pk[par][2 * m][1], pk[par][2 * m + 1][1], false, false);
          u32x4 ov = {sx[0], sy[0], sx[1], sy[1]};
          __builtin_amdgcn_raw_buffer_store_b128(ov, r16, off[par] + (nt * 32 + 16 * m) * 2, 0, 0);
        }
      }
    }
  }
}

// The tile shapes that run two blocks per CU (8 rows): one tile per block; a second block covers the first one's prologue and epilogue.
template <int TH, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2)
void conv3x3_wino_kernel(ConvArgs p, int tiles_x, int n_tiles) {
  using S = WinoShape<TH, BN, WM, WN>;
  constexpr int MT = S::MT, NT = S::NT, G = S::G, SL = S::SL;
  constexpr int PF_TAP = 5;                  // tap at which the next chunk's raw rows are requested; they are parked at tap 10
  static_assert(TH == 8, "two blocks per CU: the 8-row shapes only");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  int bid = blockIdx.x;
  const int ntile = bid % n_tiles;
  bid /= n_tiles;
  const int tx = bid % tiles_x, ty = bid / tiles_x;
  const int b = blockIdx.y;
  const int y0 = ty * TH, x0 = tx * TW, n0 = ntile * BN;

  const int Hin = p.upsample ? p.H / 2 : p.H;
  const int Win = p.upsample ? p.W / 2 : p.W;
  const half_t* xb = p.x + (size_t)b * Hin * Win * p.Cin;
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.w_wino, 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, 0x7FFFFFFF, 0x00020000);

  // ---- loader
  const int lpr = tid / G, ls = tid % G;
  unsigned row_off[4], col_off[SL], dst_off[SL];
  bool slot_ok[SL];
  wino_row_offsets(p, Win, y0, lpr, row_off);
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    const int slot = ls + j * G;
    slot_ok[j] = slot < 72;
    col_off[j] = wino_col_offset(p, x0, slot);
    dst_off[j] = wino_slot_dst(lpr, slot);
  }
  u32x4 raw[SL][4];
  auto load_rows = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < SL; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        raw[j][i] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, row_off[i] + col_off[j], chunk * BK * 2, 0);
  };
  auto park_rows = [&](int buf) {             // four pieces per slot (transformed outside the predicate: inside it costs registers)
#pragma unroll
    for (int j = 0; j < SL; ++j) {
      const half8 t0 = wino_T(raw[j], 0), t1 = wino_T(raw[j], 1), t2 = wino_T(raw[j], 2), t3 = wino_T(raw[j], 3);
      if (slot_ok[j]) {
        unsigned char* d = smem + buf * S::PATCH_BYTES + dst_off[j];
        *reinterpret_cast<half8*>(d) = t0;
        *reinterpret_cast<half8*>(d + PITCH * 64) = t1;
        *reinterpret_cast<half8*>(d + 2 * PITCH * 64) = t2;
        *reinterpret_cast<half8*>(d + 3 * PITCH * 64) = t3;
      }
    }
  };

  // ---- fragments
  const int frag_px = lane & 15, frag_pr = (lane & 31) >> 4, kgrp = lane >> 5;
  int rd_base[3][2];
  wino_rd_base<MT>(rd_base, wm, frag_px, frag_pr, kgrp);
  const int c16 = p.Cin >> 4;
  unsigned wfrag[NT];
  wino_wfrag<NT>(wfrag, n0 >> 5, wn, c16, lane);
  f32x16 acc[4][NT][MT];
  f32x4 bv[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) bv[nt][rq] = *reinterpret_cast<const f32x4*>(p.bias + n0 + (wn * NT + nt) * 32 + 8 * rq + 4 * kgrp);
  wino_init_acc<MT, NT>(acc, bv);

  const int n_chunks = p.Cin / BK;             // even
  half8 wf[3][NT][2];                          // weight fragments of three taps: in use, next, the one after
  half8 bf[2][2][MT];                          // pixel fragments of two taps (both k-steps)
  auto load_w = [&](half8 (&dst)[NT][2], int tap12, int chunk) { wino_load_w<NT>(dst, w_rsrc, wfrag, wino_w_soff(c16, tap12, chunk, 0)); };
  auto read_b = [&](half8 (&dst)[2][MT], int f, int kx, int buf) { wino_read_b<MT>(dst, smem + buf * S::PATCH_BYTES, rd_base, f, kx); };

  load_rows(0);
  load_w(wf[0], 0, 0);
  load_w(wf[1], 1, 0);
  park_rows(0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  read_b(bf[0], 0, 0, 0);

#pragma unroll 1
  for (int pair = 0; pair < n_chunks; pair += 2) {
#pragma unroll
    for (int t = 0; t < 24; ++t) {
      const int tt = t % 12, chunk_i = pair + t / 12, buf = t / 12;
      const int f = tt / 3;
      const bool more = chunk_i + 1 < n_chunks;                 // uniform
      // 1) the weights of tap t + 2 (past the very end: re-read, unused)
      {
        const int t2 = (tt + 2) % 12;
        const int c2 = tt + 2 >= 12 ? (more ? chunk_i + 1 : chunk_i) : chunk_i;
        load_w(wf[(t + 2) % 3], t2, c2);
      }
      if (tt == PF_TAP && more) load_rows(chunk_i + 1);
      // 2) the pixels of tap t + 1; across the chunk boundary from the other buffer (published by the barrier of tap 10)
      if (tt != 11) read_b(bf[(t + 1) & 1], (tt + 1) / 3, (tt + 1) % 3, buf);
      else if (more) read_b(bf[(t + 1) & 1], 0, 0, buf ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      // 3) this tap's MFMAs
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[f][nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[t % 3][nt][ks], bf[t & 1][ks][mt], acc[f][nt][mt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // 4) the next chunk's patch: parked in the other buffer, published for tap 11's reads
      if (tt == 10 && more) {
        park_rows(buf ^ 1);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
  }

  wino_epilogue<MT, NT>(p, acc, b, y0, x0, n0, wm, wn, frag_px, frag_pr, kgrp, p.relu);
}

// The interleaved schedule, for ONE wave per SIMD (the 16-row tiles: 256 accumulator registers per lane in AGPRs).  Nothing but the wave's
// own instruction order hides a latency there, so every MFMA is followed by its share of the tap's other work in SOURCE order,
// pinned by a sched_barrier: the weight loads of tap t + 3, the pixel reads of tap t + 1, and the staging of the next chunk's
// patch spread over the taps (raw rows requested slot by slot at taps 2.., transformed and parked slot by slot at taps 7.., one
// barrier after tap 10).
// A block WALKS its tiles: tile blockIdx.x, blockIdx.x + gridDim.x, .. below n_total of the linear order (channel tile fastest,
// then tx, ty, the image) -- a list fixed at entry: no counter, no atomics, nothing between blocks.  The one branch of the loop body,
// uniform and once per pair of chunks, points the staging of a tile's LAST chunk at chunk 0 of the next tile (the slot in which a
// lone tile stages a patch nobody reads): when the epilogue starts, the next patch is parked in buffer 0 and the next tile's first
// three taps of weights are in flight, so only the block's first tile has a prologue.  Every output keeps its accumulation order.
template <int TH, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 1)
void conv3x3_wino_walk_kernel(ConvArgs p, int tiles_x, int n_tiles, int tiles_y, int n_total) {
  using S = WinoShape<TH, BN, WM, WN>;
  constexpr int MT = S::MT, NT = S::NT, G = S::G, SL = S::SL;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the thread index made again from the wave's number (a scalar) and the lane's position in the wave, as a copy the compiler cannot
  // see through: what is derived from it is computed where it is written, and no vector register carries it through the chunk loop
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  auto fresh_tid = [&]() {
    int v;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(v));
    return wave_s * 64 + v;
  };
  const int wm = wave / WN, wn = wave % WN;
  // a tile of the linear order: channel tile fastest, then tx, ty, the image
  struct Tile { int b, y0, x0, n0; };
  auto tile_at = [&](int t) {
    Tile r;
    r.n0 = (t % n_tiles) * BN;
    t /= n_tiles;
    r.x0 = (t % tiles_x) * TW;
    t /= tiles_x;
    r.y0 = (t % tiles_y) * TH;
    r.b = t / tiles_y;
    return r;
  };
  Tile cur = tile_at(blockIdx.x);

  const int Hin = p.upsample ? p.H / 2 : p.H;
  const int Win = p.upsample ? p.W / 2 : p.W;
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.w_wino, 0, 0x7FFFFFFF, 0x00020000);
  auto image_rsrc = [&](int b) { return __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (size_t)b * Hin * Win * p.Cin), 0, 0x7FFFFFFF, 0x00020000); };
  __amdgpu_buffer_rsrc_t x_rsrc = image_rsrc(cur.b);

  // ---- loader
  const int lpr = tid / G, ls = tid % G;
  unsigned row_off[4], col_off[SL], dst_off[SL];
  bool slot_ok[SL];
  auto stage_from = [&](int y0, int x0) {      // the raw rows and columns of the patch of the tile at (y0, x0)
    const int tid_s = fresh_tid(), lpr = tid_s / G, ls = tid_s % G;
    wino_row_offsets(p, Win, y0, lpr, row_off);
#pragma unroll
    for (int j = 0; j < SL; ++j) col_off[j] = wino_col_offset(p, x0, ls + j * G);
  };
  stage_from(cur.y0, cur.x0);
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    const int slot = ls + j * G;
    slot_ok[j] = slot < 72;
    dst_off[j] = wino_slot_dst(lpr, slot);
    if (!slot_ok[j]) dst_off[j] = S::DUMP_OFF + tid * 16;        // (no exec-mask branch in the interleaved loop)
  }
  u32x4 raw[SL][4];
  auto load_rows = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < SL; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        raw[j][i] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, row_off[i] + col_off[j], chunk * BK * 2, 0);
  };

  // ---- fragments
  const int frag_px = lane & 15, frag_pr = (lane & 31) >> 4, kgrp = lane >> 5;
  int rd_base[3][2];
  wino_rd_base<MT>(rd_base, wm, frag_px, frag_pr, kgrp);
  const int c16 = p.Cin >> 4;
  unsigned wfrag[NT];
  wino_wfrag<NT>(wfrag, 0, wn, c16, lane);
  // the channel tile's share of the weight address is uniform and rides in the scalar offset, so it changes with the tile for free
  auto wtile_off = [&](int n0) { return (unsigned)((n0 >> 5) * 12 * c16 * 1024); };

  f32x16 acc[4][NT][MT];
  const int n_chunks = p.Cin / BK;             // even
  half8 bf[3][2][MT];                          // pixel fragments of three taps (both k-steps): read two taps ahead

  // ---- the block's tiles
  int tile = blockIdx.x;
  Tile nxt = cur;
  unsigned wt_cur = wtile_off(cur.n0), wt_nxt = wt_cur;
  bool has_next = false;
  constexpr int WR = 4, WA = WR - 1;           // weight fragments of WR taps: loaded WA taps ahead (WR divides 24)
  static_assert(24 % WR == 0, "ring");
  half8 wq[WR][NT][2];
  half8 tq[4];                                   // the transformed pieces of the slot being parked
  {
    // the block's first tile: the only one with a prologue (the later ones find patch, weights and pixels where the loop left them)
    load_rows(0);
#pragma unroll
    for (int i = 0; i < WA; ++i) wino_load_w<NT>(wq[i], w_rsrc, wfrag, wino_w_soff(c16, i, 0, wt_cur));
    // (first patch: every slot valid or dumped -- the plain park with the predicate replaced by the dump address)
#pragma unroll
    for (int j = 0; j < SL; ++j) {
      unsigned char* d = smem + dst_off[j];
      *reinterpret_cast<half8*>(d) = wino_T(raw[j], 0);
      *reinterpret_cast<half8*>(d + PITCH * 64) = wino_T(raw[j], 1);
      *reinterpret_cast<half8*>(d + 2 * PITCH * 64) = wino_T(raw[j], 2);
      *reinterpret_cast<half8*>(d + 3 * PITCH * 64) = wino_T(raw[j], 3);
    }
    for (int c = tid * 4; c < p.Cout; c += 1024) *reinterpret_cast<f32x4*>(smem + S::BIAS_OFF + c * 4) = *reinterpret_cast<const f32x4*>(p.bias + c);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
#pragma unroll 1
  for (;;) {
  {
    constexpr int NM = 2 * MT * NT;              // MFMAs of a tap
    constexpr int NR = 2 * NT + 2 * MT;          // its regular fillers: weight loads (tap t + 3), pixel reads (tap t + 1)
    constexpr int LT0 = 1, PT0 = 6;              // staging: slot s is requested at tap LT0 + s, parked at tap PT0 + s; barrier after tap 9
    static_assert(LT0 + SL <= PT0 && PT0 + SL <= 10, "staging schedule");
    has_next = tile + (int)gridDim.x < n_total;
    // a tile starts from LDS alone: its first patch is in buffer 0 (parked by the prologue or by the previous tile's last chunk) and
    // its taps 0..2 are in the weight ring; the pixel fragments of taps 0 and 1 are read again here instead of being carried in 64
    // registers across the epilogue
    wino_read_b<MT>(bf[0], smem, rd_base, 0, 0);
    wino_read_b<MT>(bf[1], smem, rd_base, 0, 1);
    {
      // the bias in M1 first, as ever; from the copy in LDS (made once per block), so that a later tile's bias does not queue behind
      // the previous tile's stores
      const int tid_b = fresh_tid(), wn = (tid_b >> 6) % WN, kgrp = (tid_b & 63) >> 5;
      f32x4 bv[NT][4];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) bv[nt][rq] = *reinterpret_cast<const f32x4*>(smem + S::BIAS_OFF + (cur.n0 + (wn * NT + nt) * 32 + 8 * rq + 4 * kgrp) * 4);
      wino_init_acc<MT, NT>(acc, bv);
    }
#pragma unroll 1
    for (int pair = 0;;) {                       // (n_chunks >= 2: Cin is a multiple of 64)
      // what the pair's second chunk stages: the chunk after it; past the tile's end chunk 0 of the block's next tile -- the loop
      // leaves that tile's first patch in buffer 0 (n_chunks is even), its taps 0..2 in the weight ring and its taps 0, 1 in the
      // pixel ring, which is where the prologue puts the first tile's -- or, on the block's last tile, itself (nobody reads it)
      int stage_c = pair + 2;
      unsigned stage_wt = wt_cur;
#pragma unroll
      for (int t = 0; t < 24; ++t) {
        const int tt = t % 12, chunk_i = pair + t / 12, buf = t / 12;
        const int f = tt / 3;
        if (t == 12 && pair + 2 >= n_chunks) {     // uniform, once per pair: the last raw rows of this tile were requested at tap 3
          stage_c = pair + 1;
          if (has_next) {
            nxt = tile_at(tile + (int)gridDim.x);
            stage_c = 0;
            stage_wt = wt_nxt = wtile_off(nxt.n0);
            stage_from(nxt.y0, nxt.x0);            // (the current tile's offsets are dead: overwritten, not doubled)
            x_rsrc = image_rsrc(nxt.b);
          }
        }
        const int chunk_n = t < 12 ? pair + 1 : stage_c;
        const unsigned wt_n = t < 12 ? wt_cur : stage_wt;
        const int t3 = (tt + WA) % 12, c3 = tt + WA >= 12 ? chunk_n : chunk_i;
        const int t1 = (tt + 2) % 12, buf1 = tt >= 10 ? buf ^ 1 : buf;        // (the pixel reads run two taps ahead)
        const int soff3 = wino_w_soff(c16, t3, c3, tt + WA >= 12 ? wt_n : wt_cur);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
          const int ks = j / (MT * NT), mt = (j / NT) % MT, nt = j % NT;
          acc[f][nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[t % WR][nt][ks], bf[t % 3][ks][mt], acc[f][nt][mt], 0, 0, 0);
#pragma unroll
          for (int k = j * NR / NM; k < (j + 1) * NR / NM; ++k) {
            if (k < 2 * NT) {
              wq[(t + WA) % WR][k / 2][k % 2] = wino_weight_frag(w_rsrc, wfrag[k / 2], k % 2, soff3);
            } else {
              const int kk = k - 2 * NT, ks1 = kk / MT, mt1 = kk % MT;
              bf[(t + 2) % 3][ks1][mt1] = wino_pixel_frag(smem + buf1 * S::PATCH_BYTES, rd_base, t1 / 3, t1 % 3, ks1, mt1);
            }
          }
          if (tt >= LT0 && tt < LT0 + SL) {            // one slot's four raw rows: a load behind each of the first four MFMAs
            const int sl = tt - LT0;
            if (j < 4) raw[sl][j] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, row_off[j] + col_off[sl], chunk_n * BK * 2, 0);
          }
          if (tt >= PT0 && tt < PT0 + SL) {            // one slot parked: a transformed piece, then its store, per pair of MFMAs
            const int sl = tt - PT0;
#pragma unroll
            for (int it = j * 8 / NM; it < (j + 1) * 8 / NM; ++it) {          // 8 items over the tap's MFMAs
              const int fq = it >> 1;
              if ((it & 1) == 0) tq[fq] = wino_T(raw[sl], fq);
              else *reinterpret_cast<half8*>(smem + (buf ^ 1) * S::PATCH_BYTES * (slot_ok[sl] ? 1 : 0) + dst_off[sl] + fq * PITCH * 64) = tq[fq];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (tt == 9) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      if ((pair += 2) >= n_chunks) break;
    }
  }
  // ---- epilogue.  The next tile's first patch is parked, its first weight and pixel fragments and its bias are in registers or in
  // flight -- all requested BEFORE these stores (vmcnt counts in order: a wait for a load issued after a store waits for the store too).
  // (the lane's coordinates are derived again from the thread index, behind an opaque copy of it: hoisted out of the tile loop
  // they would have to live through the chunk loop, which has no register to spare, and end in scratch)
  const int tid_e = fresh_tid();
  const int lane_e = tid_e & 63, wn = (tid_e >> 6) % WN, wm = (tid_e >> 6) / WN;
  int relu = p.relu;
  asm volatile("" : "+s"(relu));      // (the ReLU floor is a vector value: made in the epilogue, not carried around the tile loop)
  wino_epilogue<MT, NT>(p, acc, cur.b, cur.y0, cur.x0, cur.n0, wm, wn, lane_e & 15, (lane_e & 31) >> 4, lane_e >> 5, relu);
  if (!has_next) break;
  tile += gridDim.x;
  cur = nxt;
  wt_cur = wt_nxt;
  }     // the block's tiles
}

template <int TH, int BN, int WM, int WN>
int launch_wino_cfg(const ConvArgs& a, hipStream_t s) {
  const int tiles_x = cdiv(a.W, TW), tiles_y = cdiv(a.H, TH), n_tiles = a.Cout / BN;
  const size_t lds = WinoShape<TH, BN, WM, WN>::patch_lds_bytes();
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wino_kernel<TH, BN, WM, WN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((conv3x3_wino_kernel<TH, BN, WM, WN>), dim3(tiles_x * tiles_y * n_tiles, a.B), dim3(256), lds, s, a, tiles_x, n_tiles);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// The walking kernel: min(total tiles, CUs of the device) blocks in one grid dimension, block g on the tiles g, g + grid, ..
template <int TH, int BN, int WM, int WN>
int launch_wino_walk(const ConvArgs& a, hipStream_t s) {
  const int tiles_x = cdiv(a.W, TW), tiles_y = cdiv(a.H, TH), n_tiles = a.Cout / BN;
  const long total = (long)tiles_x * tiles_y * n_tiles * a.B;
  const size_t lds = WinoShape<TH, BN, WM, WN>::lds_bytes(a.Cout);       // patches, dump area, bias
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  ARG_CHECK(cus > 0 && total < (1L << 30) && lds <= 160 * 1024);
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wino_walk_kernel<TH, BN, WM, WN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((conv3x3_wino_walk_kernel<TH, BN, WM, WN>), dim3((unsigned)(total < cus ? total : cus)), dim3(256), lds, s, a, tiles_x,
                     n_tiles, tiles_y, (int)total);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

// The layers this kernel takes (launch_conv3x3 asks): fp16 output only (no fp32 tap, no statistics, no conv1_1 in the loader).
// Every tile shape accumulates in the same order (chunk, f, kx, k-step), so the choice below -- made from the grid size, like
// launch_conv3x3's -- does not change a bit of the output: batch 32 == single pair holds.
bool conv3x3_wino_takes(const ConvArgs& a) {
  return a.w_wino != nullptr && a.y16 != nullptr && a.y32 == nullptr && a.usum == nullptr && a.img1 == nullptr &&
         a.Cin % 64 == 0 && a.Cout % 64 == 0 && (!a.pool || a.relu);
}

int launch_conv3x3_wino(const ConvArgs& a, hipStream_t s) {
  ARG_CHECK(conv3x3_wino_takes(a) && a.H > 1 && a.W > 1 && a.B > 0);
  ARG_CHECK(!a.upsample || (a.H % 2 == 0 && a.W % 2 == 0));
  ARG_CHECK(launch_map_fits((size_t)a.H * a.W * a.Cin, 2));
  ARG_CHECK(launch_map_fits((size_t)a.H * a.W * a.Cout, 2));
  const long px16 = (long)cdiv(a.W, TW) * cdiv(a.H, 16) * a.B;
  // one block per CU with the interleaved schedule, walking its 256-pixel x 128-channel tiles, where the tiles fill the chip; below,
  // blocks of 8 rows at two per CU, one tile each (the second block covers the first one's prologue and epilogue)
  const long px8 = (long)cdiv(a.W, TW) * cdiv(a.H, 8) * a.B;
  if (a.Cout % 128 == 0 && px16 * (a.Cout / 128) >= 256) return launch_wino_walk<16, 128, 1, 4>(a, s);
  if (a.Cout % 128 == 0 && px8 * (a.Cout / 128) >= 256) return launch_wino_cfg<8, 128, 1, 4>(a, s);
  return launch_wino_cfg<8, 64, 2, 2>(a, s);
}
