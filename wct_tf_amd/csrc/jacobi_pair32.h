// The 32-wide block pairs of the batched block-Jacobi eigensolver (C <= 128, and every C that is no multiple of 64): the device
// code of jacobi_fused_kernel (eigh.hip).  A pair problem is the M2 x M2 symmetric matrix of two column blocks of B = M2 / 2;
// B x B threads hold it in LDS as an image of float2 {S[r][c], Q[r][c]} -- S the problem, Q the accumulated rotations -- so that
// thread (k, l) moves its 2 x 2 block of both (rows {p_k, q_k} x columns {p_l, q_l}) with four 8-byte LDS reads and writes per
// rotation set, B disjoint pairs per set.  A cross step rotates the B^2 pairs (i in block I, j in block J) in B sets
// (cross_sets), the intra step the pairs inside I and inside J in B - 1 sets (intra_sets), so that one outer sweep visits every
// pair of the C indices exactly once: a true cyclic Jacobi sweep.  The D and U parts of a look-ahead launch: fused_d, fused_u.
#pragma once
#include <type_traits>
#include "jacobi_dev.h"

namespace pair32 {
constexpr int M2 = 32, B = M2 / 2;         // pair width, block width
constexpr int NT = B * B;                  // 256 threads per pair problem / per update task: thread (k, l) of the B x B grid
constexpr int NW = M2 / 16;                // 16 x 16 MFMA tiles along a side of the pair problem; NW x NW = the block's 4 waves
constexpr int NCH = M2 / 32;               // K-chunks of a fp16 fragment (qfrag16_k)

// The sets of a cross step: set s pairs p_j = j with q_j = B + ((j + s) mod B).  ONE wave carries the rotation parameters
// (the "pivot wave") -- derived by every thread for its own column pair, a rotation is ~35 instructions with three
// transcendentals on a dependent chain, 16x redundant.  Here:
//   * threads are numbered along the diagonals of the (k, l) grid: k = t % B, d = t / B, l = k + d + 1 (mod B), so the
//     B threads (k, k+1) that own S[p_k][q_k'] -- the element pair k annihilates in the NEXT set -- are the first B
//     lanes of wave 0;
//   * those lanes keep pair k's pivot block (pp, qq, pq) in registers: pp and qq follow in closed form from the
//     rotation they computed for this set (c^2 pp - 2cs pq + s^2 qq, ...), the q diagonal of pair k+1 arrives by one
//     lane shift, pq is their own freshly rotated element; they derive the next rotation and publish (c, s) in a
//     ping-pong LDS array; every other wave reads (c_l, s_l), (c_k, s_k) -- two 8-byte loads -- and only rotates;
//   * within a set every element of the {S, Q} image is read and written by exactly one thread, so the image is
//     updated in place (one image, one barrier per set); with a pitch of M2 the 8-byte accesses of a diagonal are conflict-free.
// Per set a bulk wave issues ~45 instructions instead of ~100, and the dependent chain of a set is the pivot wave's.
__device__ __forceinline__ void cross_sets(unsigned char* sq, unsigned char* csb, int t, float floor_m, float& my_off, float& my_sig) {
  constexpr int N = M2, NP = B, ROWB = N * 8;                        // pairs per set; bytes per image row
  constexpr int CSB = NP * 8, DUMMY = 2 * CSB;                       // csb layout: CS[2][NP] float2 (c, s), dummy float2
  const int k = t & (NP - 1), d = t / NP;
  const int l = (k + d + 1) & (NP - 1);
  const bool pwave = __builtin_amdgcn_readfirstlane(t >> 6) == 0;    // wave-uniform: the wave holding the lanes (k, k+1)
  const bool piv = d == 0;
  float ppk = 0.f, qqk = 0.f, pqk = 0.f, ck = 1.f, sk = 0.f;         // pair k's pivot block and rotation (pivot wave only)
  if (pwave) {
    __builtin_amdgcn_s_setprio(2);                                   // the chain of a set runs through this wave
    const f32x2* SQ = reinterpret_cast<const f32x2*>(sq);
    ppk = SQ[k * N + k][0]; qqk = SQ[(NP + k) * N + NP + k][0]; pqk = SQ[k * N + NP + k][0];   // set 0 pairs k with NP + k
    float off, sig;
    jacobi_rotation(ppk, qqk, pqk, floor_m, ck, sk, off, sig);
    if (piv) { my_off = fmaxf(my_off, off); my_sig = fmaxf(my_sig, sig); }
    f32x2 r; r[0] = ck; r[1] = sk;
    *reinterpret_cast<f32x2*>(csb + (piv ? k * 8 : DUMMY)) = r;
  }
  __syncthreads();
  const int row_pk = k * ROWB, col_pl = l * 8;
  const int a_pp = row_pk + col_pl;
  int qk = NP + k, ql = NP + l;                                      // q index of set s: NP + ((j + s) & (NP - 1))
  const int cs_l = l * 8, cs_k = k * 8;
  const int cs_w0 = piv ? k * 8 : DUMMY, cs_w1 = piv ? CSB + k * 8 : DUMMY;   // the dummy slot absorbs the lanes that own no pair
  auto ld2 = [&](const unsigned char* base, int off) { return *reinterpret_cast<const f32x2*>(base + off); };
  auto body = [&](auto CURC) {
    constexpr int CUR = decltype(CURC)::value, NX = CUR ^ 1;
    const f32x2 rl = ld2(csb + CUR * CSB, cs_l), rk = ld2(csb + CUR * CSB, cs_k);
    const int qlb = ql * 8, qkb = qk * ROWB;
    const int a_pq = row_pk + qlb, a_qp = qkb + col_pl, a_qq = qkb + qlb;
    const f32x2 app = ld2(sq, a_pp), apq = ld2(sq, a_pq), aqp = ld2(sq, a_qp), aqq = ld2(sq, a_qq);
    const float cl = rl[0], sl = rl[1], ckk = rk[0], skk = rk[1];
    // columns (pair l) on the {S, Q} pairs as packed operations -- the same (c_l, s_l) acts on both halves of a
    // float2, so v_pk_mul / v_pk_fma take the scalars broadcast and need no operand assembly --, then rows (pair k) on
    // the S halves alone.  (Written element by element the same arithmetic came out of hipcc as 12 packed operations
    // fed by ~30 v_mov: the set loop is VALU-issue bound, ablation in profiles/r03_jacobi_set_ablation.txt.)
    const f32x2 ypp = cl * app - sl * apq, ypq = sl * app + cl * apq;
    const f32x2 yqp = cl * aqp - sl * aqq, yqq = sl * aqp + cl * aqq;
    f32x2 npp = ypp, npq = ypq, nqp = yqp, nqq = yqq;
    npp[0] = ckk * ypp[0] - skk * yqp[0];  npq[0] = ckk * ypq[0] - skk * yqq[0];
    nqp[0] = skk * ypp[0] + ckk * yqp[0];  nqq[0] = skk * ypq[0] + ckk * yqq[0];
    if (pwave) {
      // pair k after this set's rotation (closed form from registers), the next set's partner diagonal from the
      // lane of pair k+1 -- a DPP wave shift (lane i reads lane i+1), the wrap-around lane NP-1 <- 0 patched with a
      // v_readlane: no LDS round trip on the chain --, the next pivot element from this thread's own block
      const float c2 = ck * ck, s2 = sk * sk, cs2 = 2.f * ck * sk;
      const float ppn = c2 * ppk - cs2 * pqk + s2 * qqk;
      const float qqn = s2 * ppk + cs2 * pqk + c2 * qqk;
      const int qqn_i = __builtin_bit_cast(int, qqn);
      const int shl = __builtin_amdgcn_update_dpp(qqn_i, qqn_i, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
      const int first = __builtin_amdgcn_readlane(qqn_i, 0);
      const float qq_next = __builtin_bit_cast(float, k == NP - 1 ? first : shl);
      ppk = ppn; qqk = qq_next; pqk = npq[0];
      const bool rot = jacobi_rotation_cs(ppk, qqk, pqk, ck, sk);
      f32x2 r; r[0] = ck; r[1] = sk;
      *reinterpret_cast<f32x2*>(csb + (NX ? cs_w1 : cs_w0)) = r;
      float off, sig;
      jacobi_rotation_stats(ppk, qqk, pqk, floor_m, rot, off, sig);
      if (piv) { my_off = fmaxf(my_off, off); my_sig = fmaxf(my_sig, sig); }
    }
    *reinterpret_cast<f32x2*>(sq + a_pp) = npp;  *reinterpret_cast<f32x2*>(sq + a_pq) = npq;
    *reinterpret_cast<f32x2*>(sq + a_qp) = nqp;  *reinterpret_cast<f32x2*>(sq + a_qq) = nqq;
    qk = NP | ((qk + 1) & (NP - 1));
    ql = NP | ((ql + 1) & (NP - 1));
    __syncthreads();
  };
#pragma unroll 1
  for (int s = 0; s < NP; s += 2) {
    body(std::integral_constant<int, 0>{});
    body(std::integral_constant<int, 1>{});
  }
}

// The sets of the intra step: the pairs inside block I and inside block J, round-robin (circle method) within each, B / 2
// pairs per block and set, B - 1 sets.  Pair j of set s:
__device__ __forceinline__ void intra_pair(int j, int s, int& p, int& q) {
  const int base = j & (B / 2) ? B : 0, jj = j & (B / 2 - 1);
  p = base + rr_idx(jj, s, B);
  q = base + rr_idx(B - 1 - jj, s, B);
}
// Thread t = (k, l) = (t / B, t % B).  The partners change from set to set, so two LDS images (pitch M2 + 1) ping-pong and a
// set costs ONE barrier.  Each thread derives rotation(l) from three more reads of the image; rotation(k) is fetched from the
// lane of its own wave that has l == k (a lane shuffle: no serial section).  All threads of the block call this together
// (contains __syncthreads()).  Returns the index of the image that holds the result.
// A thread has ONE cell; the cell's reads and its arithmetic stand in loops `for (i < CELLS)` all the same: written straight,
// hipcc addresses the set loop differently (2433 -> 2443 instruction lines, profiles/eigh_widths_isa.txt).
__device__ __forceinline__ int intra_sets(f32x2* SQ, int t, float floor_m, float& my_off, float& my_sig) {
  constexpr int CELLS = 1, PITCH = M2 + 1, IMG = M2 * PITCH;
  const int k = t / B, l = t % B;
  int cur = 0;
  for (int s = 0; s < B - 1; ++s) {
    int pl, ql;
    intra_pair(l, s, pl, ql);
    const f32x2* C0 = SQ + cur * IMG;
    f32x2* N0 = SQ + (cur ^ 1) * IMG;
    // every LDS read of the set is issued before anything depends on it
    float lpp, lqq, lpq;
    lpp = C0[pl * PITCH + pl][0]; lqq = C0[ql * PITCH + ql][0]; lpq = C0[pl * PITCH + ql][0];
    int pk[CELLS], qk[CELLS];
    f32x2 app[CELLS], apq[CELLS], aqp[CELLS], aqq[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; ++i) {
      intra_pair(k, s, pk[i], qk[i]);
      app[i] = C0[pk[i] * PITCH + pl]; apq[i] = C0[pk[i] * PITCH + ql];
      aqp[i] = C0[qk[i] * PITCH + pl]; aqq[i] = C0[qk[i] * PITCH + ql];
    }
    float cl, sl, offl, sigl;
    jacobi_rotation(lpp, lqq, lpq, floor_m, cl, sl, offl, sigl);
    my_off = fmaxf(my_off, offl);
    my_sig = fmaxf(my_sig, sigl);
#pragma unroll
    for (int i = 0; i < CELLS; ++i) {
      const int src_lane = (t & (64 - B)) | k;      // lane of my wave whose l equals this k
      const float ck = __shfl(cl, src_lane, 64), sk = __shfl(sl, src_lane, 64);
      // S: columns (pair l), then rows (pair k);  Q: columns only
      const float ypp = cl * app[i][0] - sl * apq[i][0], ypq = sl * app[i][0] + cl * apq[i][0];
      const float yqp = cl * aqp[i][0] - sl * aqq[i][0], yqq = sl * aqp[i][0] + cl * aqq[i][0];
      f32x2 npp, npq, nqp, nqq;
      npp[0] = ck * ypp - sk * yqp;  npq[0] = ck * ypq - sk * yqq;
      nqp[0] = sk * ypp + ck * yqp;  nqq[0] = sk * ypq + ck * yqq;
      npp[1] = cl * app[i][1] - sl * apq[i][1];  npq[1] = sl * app[i][1] + cl * apq[i][1];
      nqp[1] = cl * aqp[i][1] - sl * aqq[i][1];  nqq[1] = sl * aqp[i][1] + cl * aqq[i][1];
      N0[pk[i] * PITCH + pl] = npp;  N0[pk[i] * PITCH + ql] = npq;
      N0[qk[i] * PITCH + pl] = nqp;  N0[qk[i] * PITCH + ql] = nqq;
    }
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// ---------------------------------------------------------------------------
// Look-ahead launches.  The serial chain of a solve would be  D(s) -> U(s) -> D(s+1) -> ...  (pair problems, then the
// tile update that needs their rotations, then the next pair problems that need the updated tiles): two dependent
// launches per outer step, the latency-bound pair problems idle while the tile update runs and vice versa.  Instead ONE
// launch carries  { D(s), U(s-1) }:
//   * D(s) does not wait for U(s-1).  Its 2B x 2B pair problem (blocks bi, bj) is assembled from the rotated images
//     D(s-1) left behind (Sbuf: they ARE the diagonal tiles after U(s-1)) and ONE off-diagonal B x B block it
//     computes itself -- crit = Q_g1[:, h1]^T . P_old[tile g1, g2] . Q_g2[:, h2], with (g1, h1) / (g2, h2) the pair and
//     half that held bi / bj at step s-1 -- from the matrix state BEFORE U(s-1) and the rotations of step s-1;
//   * U(s-1) reads P_old and writes every tile into the other buffer P_new (off-diagonal tiles g < h computed and
//     mirrored, diagonal tiles copied from Sbuf), so D(s) can read P_old while it runs; V is updated in place.
// Both parts use the whole block, NT threads = NW x NW waves, one 16x16 output tile of v_mfma_f32_16x16x4_f32 per wave.
// The chain of a solve becomes D -> D -> D ...; the tile updates run beside it.
// Data routing checked against the plain sequence in tools/jacobi_lookahead_proto.py.
// ---------------------------------------------------------------------------

// dynamic LDS of one launch (every block of a launch gets the same amount: the larger of its D and U parts)
constexpr size_t lds_bytes(int has_d, int has_u, int first, int step_d) {
  constexpr size_t F = sizeof(float);
  // intra sets: two images, and 4 M2 floats behind them that nothing has used since the pivot wave took over the cross sets
  // (they held mirrors of the pivots).  Kept: the LDS of a launch is part of how it is scheduled.
  constexpr size_t intra = 2 * M2 * (M2 + 1) * sizeof(f32x2) + 4 * M2 * F;
  constexpr size_t cross = M2 * M2 * sizeof(f32x2) + (M2 + 2) * sizeof(f32x2);          // one image, CS[2][B], dummy
  constexpr size_t ahead = (M2 * (M2 + 1) + 2 * M2 * (B + 1) + B * (M2 + 1)) * F;       // look-ahead staging: Xs, Q1s, Q2s, Ws
  constexpr size_t update = 3 * M2 * (M2 + 1) * F;                                      // Xs, Qhs, Qgs
  size_t need = 0;
  if (has_d) need = step_d < 0 ? intra : (!first && ahead > cross ? ahead : cross);
  if (has_u && need < update) need = update;
  return need;
}
static_assert(lds_bytes(1, 0, 1, -1) == 17408 && lds_bytes(1, 0, 1, 0) == 8464 && lds_bytes(1, 0, 0, 0) == 10688 &&
              lds_bytes(0, 1, 0, 0) == 12672 && lds_bytes(1, 1, 0, 0) == 12672, "LDS of the launches of the 32-wide kernel");

__device__ __forceinline__ void fused_d(const JacobiFusedArgs& p, int m, int g, float* jsm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.C, nblk = C / B, npair = nblk / 2;
  f32x2* SQ = reinterpret_cast<f32x2*>(jsm);
  int bi, bj;
  block_pair(g, p.step_d, nblk, bi, bj);
  // the matrix' state words (done, floor) are read AFTER the block's data loads have been issued: a done matrix costs a few
  // wasted loads, a live one does not wait a memory round trip before it requests anything
  float floor_m = 0.f;
  float my_off = 0.f, my_sig = 0.f, my_dm = 0.f;
  bool finite = true;
  float* Qo = p.Qw + ((size_t)m * npair + g) * (M2 * M2);
  float* So = p.Sw + ((size_t)m * npair + g) * (M2 * M2);
  if (p.first) {
    if (p.st[m].done) return;
    floor_m = p.st[m].floor;
    const float* Am = p.Pr + (size_t)m * C * C;
    const int PITCH = p.step_d >= 0 ? M2 : M2 + 1;
    for (int e = tid; e < M2 * M2; e += NT) {
      const int r = e / M2, c = e % M2;
      f32x2 v;
      v[0] = Am[(size_t)pair_index<B>(r, bi, bj) * C + pair_index<B>(c, bi, bj)];
      v[1] = r == c ? 1.f : 0.f;
      finite &= fabsf(v[0]) <= 3.0e38f;
      if (r == c) my_dm = fmaxf(my_dm, fabsf(v[0]));
      SQ[r * PITCH + c] = v;
    }
    __syncthreads();
  } else {
    // ---- look-ahead assembly (cross steps only: a segment never starts behind an intra step)
    int g1, h1, g2, h2;
    block_locate(bi, p.step_u, nblk, g1, h1);
    block_locate(bj, p.step_u, nblk, g2, h2);
    const float* S1 = p.Sr + ((size_t)m * npair + g1) * (M2 * M2);
    const float* S2 = p.Sr + ((size_t)m * npair + g2) * (M2 * M2);
    const bool same = g1 == g2;
    // this thread's four image elements that come out of the previous images (requested before the staging loads)
    float sv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * NT, r = e / M2, c = e % M2;
      const bool rlo = r < B, clo = c < B;
      const float* src = rlo ? S1 : S2;
      const int rr = (rlo ? h1 : h2) * B + (rlo ? r : r - B);
      const int cc = (clo ? h1 : h2) * B + (clo ? c : c - B);
      sv[i] = (rlo == clo || same) ? src[rr * M2 + cc] : 0.f;
    }
    float* Xs = jsm;                                // [M2][M2 + 1]  tile (g1, g2) of the state before U(step_u)
    float* Q1s = Xs + M2 * (M2 + 1);                // [M2][B + 1]   columns h1 of Q_g1
    float* Q2s = Q1s + M2 * (B + 1);                // [M2][B + 1]   columns h2 of Q_g2
    float* Ws = Q2s + M2 * (B + 1);                 // [B][M2 + 1]   Q_g1[:, h1]^T X
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, qv = {0.f, 0.f, 0.f, 0.f};
    const int se = tid * 4, sr = se / M2, sc = se % M2;
    float* Qdst = nullptr;
    if (!same) {
      int b1i, b1j, b2i, b2j;
      block_pair(g1, p.step_u, nblk, b1i, b1j);
      block_pair(g2, p.step_u, nblk, b2i, b2j);
      const float* Pm = p.Pr + (size_t)m * C * C;
      xv = *reinterpret_cast<const f32x4*>(Pm + (size_t)pair_index<B>(sr, b1i, b1j) * C + pair_index<B>(sc, b2i, b2j));
      // Q columns: M2 x B floats per side = NT / 2 float4 (the fragments mt of that half); first half of the block
      // fetches Q_g1, second half Q_g2
      const bool one = tid < NT / 2;
      const int t2 = one ? tid : tid - NT / 2;
      const int f = (one ? h1 : h2) * (NT / 2) + t2;
      int qr, qc;
      qfrag_rc<M2>(f, qr, qc);
      qc -= (one ? h1 : h2) * B;
      qv = *reinterpret_cast<const f32x4*>(p.Qr + ((size_t)m * npair + (one ? g1 : g2)) * (M2 * M2) + (size_t)f * 4);
      Qdst = (one ? Q1s : Q2s) + qr * (B + 1) + qc;
    }
    if (p.st[m].done) return;        // (block-uniform)
    floor_m = p.st[m].floor;
    f32x4 crit = {0.f, 0.f, 0.f, 0.f};
    if (!same) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { Xs[sr * (M2 + 1) + sc + j] = xv[j]; Qdst[j * (B + 1)] = qv[j]; }
      __syncthreads();
      const int li = lane & 15, lq = lane >> 4;
      if (wave < (B / 16) * NW) {                   // W = Q_g1[:, h1]^T X   (B x M2)
        const int tr = wave / NW, tj = wave % NW;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int kk = 0; kk < M2; kk += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Q1s[(kk + lq) * (B + 1) + 16 * tr + li], Xs[(kk + lq) * (M2 + 1) + 16 * tj + li], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Ws[(16 * tr + 4 * lq + r) * (M2 + 1) + 16 * tj + li] = acc[r];
      }
      __syncthreads();
      if (wave < (B / 16) * (B / 16)) {             // crit = W Q_g2[:, h2]   (B x B)
        const int tr = wave / (B / 16), tc = wave % (B / 16);
#pragma unroll 4
        for (int kk = 0; kk < M2; kk += 4)
          crit = __builtin_amdgcn_mfma_f32_16x16x4f32(Ws[(16 * tr + li) * (M2 + 1) + kk + lq], Q2s[(kk + lq) * (B + 1) + 16 * tc + li], crit, 0, 0, 0);
      }
      __syncthreads();                              // the staging area becomes the image
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * NT, r = e / M2, c = e % M2;
      if ((r < B) == (c < B) || same) {
        f32x2 v; v[0] = sv[i]; v[1] = r == c ? 1.f : 0.f;
        SQ[e] = v;
        finite &= fabsf(sv[i]) <= 3.0e38f;
        if (r == c) my_dm = fmaxf(my_dm, fabsf(sv[i]));
      }
    }
    if (!same && wave < (B / 16) * (B / 16)) {
      const int tr = wave / (B / 16), tc = wave % (B / 16), li = lane & 15, lq = lane >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * tr + 4 * lq + r, col = B + 16 * tc + li;
        f32x2 v; v[0] = crit[r]; v[1] = 0.f;
        SQ[row * M2 + col] = v;
        SQ[col * M2 + row] = v;
        finite &= fabsf(crit[r]) <= 3.0e38f;
      }
    }
    __syncthreads();
  }
  if (p.step_d >= 0) {
    cross_sets(reinterpret_cast<unsigned char*>(SQ), reinterpret_cast<unsigned char*>(jsm + 2 * M2 * M2), tid, floor_m, my_off, my_sig);
    for (int e = tid; e < M2 * M2; e += NT) So[e] = SQ[e][0];
    int qr, qc;
    qfrag_rc<M2>(tid, qr, qc);                      // NT float4 = one tile, fragment order
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = SQ[(qr + j) * M2 + qc][1];
    *reinterpret_cast<f32x4*>(Qo + (size_t)tid * 4) = q;
    {  // fp16 hi / lo fragment unit `tid`
      const int l16 = tid & 63, part = (tid >> 6) & 1, cc = (tid >> 7) % NCH, mt = (tid >> 7) / NCH;
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = SQ[qfrag16_k<M2>(cc, l16 >> 4, j) * M2 + 16 * mt + (l16 & 15)][1];
      half8 hi, lo;
      split_f16x8(x, hi, lo);
      *reinterpret_cast<half8*>(p.Qw16 + ((size_t)m * npair + g) * (2 * M2 * M2) + (size_t)tid * 8) = part ? lo : hi;
    }
  } else {
    constexpr int PITCH = M2 + 1;
    const int cur = intra_sets(SQ, tid, floor_m, my_off, my_sig);
    for (int e = tid; e < M2 * M2; e += NT) So[e] = SQ[cur * M2 * PITCH + (e / M2) * PITCH + (e % M2)][0];
    int qr, qc;
    qfrag_rc<M2>(tid, qr, qc);
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = SQ[cur * M2 * PITCH + (qr + j) * PITCH + qc][1];
    *reinterpret_cast<f32x4*>(Qo + (size_t)tid * 4) = q;
    {
      const int l16 = tid & 63, part = (tid >> 6) & 1, cc = (tid >> 7) % NCH, mt = (tid >> 7) / NCH;
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = SQ[cur * M2 * PITCH + qfrag16_k<M2>(cc, l16 >> 4, j) * PITCH + 16 * mt + (l16 & 15)][1];
      half8 hi, lo;
      split_f16x8(x, hi, lo);
      *reinterpret_cast<half8*>(p.Qw16 + ((size_t)m * npair + g) * (2 * M2 * M2) + (size_t)tid * 8) = part ? lo : hi;
    }
  }
  if (!finite) my_off = __builtin_inff();
  for (int o = 32; o > 0; o >>= 1) {
    my_off = fmaxf(my_off, __shfl_xor(my_off, o, 64));
    my_sig = fmaxf(my_sig, __shfl_xor(my_sig, o, 64));
    my_dm = fmaxf(my_dm, __shfl_xor(my_dm, o, 64));
  }
  if ((tid & 63) == 0) {
    if (my_off > 0.f) atomicMax(&p.st[m].offmax, __float_as_uint(my_off));
    if (my_sig > 0.f) atomicMax(&p.st[m].offsig, __float_as_uint(my_sig));
    if (my_dm > 0.f && my_dm < 3.0e38f) atomicMax(&p.st[m].dmax, __float_as_uint(my_dm));
  }
}

// tasks of one matrix: [off-diagonal tiles g < h][diagonal tile copies][V tiles (row block, column pair)]
__device__ __forceinline__ void fused_u(const JacobiFusedArgs& p, int m, int task, float* jsm) {
  constexpr int PITCH = M2 + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.C, nblk = C / B, npair = nblk / 2;
  const int n_off = npair * (npair - 1) / 2;
  const size_t cc = (size_t)C * C;
  const int e4 = tid * 4, lr = e4 / M2, lc = e4 % M2;     // this thread's float4 of a staged tile
  if (task >= n_off && task < n_off + npair) {            // diagonal tile g: the image D(step_u) left behind
    const int g = task - n_off;
    int gi, gj;
    block_pair(g, p.step_u, nblk, gi, gj);
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.Sr + ((size_t)m * npair + g) * (M2 * M2) + e4);
    *reinterpret_cast<f32x4*>(p.Pw + m * cc + (size_t)pair_index<B>(lr, gi, gj) * C + pair_index<B>(lc, gi, gj)) = v;
    return;
  }
  const bool is_v = task >= n_off;               // (V tasks exist only in launches with_v)
  int g, h;
  if (is_v) { const int t = task - n_off - npair; g = t / npair; h = t % npair; }       // g = M2-row block of V
  else { int t = task; g = 0; while (t >= npair - 1 - g) { t -= npair - 1 - g; ++g; } h = g + 1 + t; }
  int hi, hj, gi = 0, gj = 0;
  block_pair(h, p.step_u, nblk, hi, hj);
  if (!is_v) block_pair(g, p.step_u, nblk, gi, gj);
  float* Xs = jsm;
  float* Qhs = Xs + M2 * PITCH;
  float* Qgs = Qhs + M2 * PITCH;
  {
    const float* X = is_v ? p.V + m * cc : p.Pr + m * cc;
    const int gr = is_v ? g * M2 + lr : pair_index<B>(lr, gi, gj);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(X + (size_t)gr * C + pair_index<B>(lc, hi, hj));
    const f32x4 hv = *reinterpret_cast<const f32x4*>(p.Qr + ((size_t)m * npair + h) * (M2 * M2) + e4);
    f32x4 gv = {0.f, 0.f, 0.f, 0.f};
    if (!is_v) gv = *reinterpret_cast<const f32x4*>(p.Qr + ((size_t)m * npair + g) * (M2 * M2) + e4);
    int qr, qc;
    qfrag_rc<M2>(tid, qr, qc);                      // the rotations arrive in fragment order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Xs[lr * PITCH + lc + j] = xv[j];
      Qhs[(qr + j) * PITCH + qc] = hv[j];
      if (!is_v) Qgs[(qr + j) * PITCH + qc] = gv[j];
    }
  }
  __syncthreads();
  const int ti = wave / NW, tj = wave % NW, li = lane & 15, lq = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (is_v) {
    // (V Qh)^T = Qh^T V^T tile (column tile tj, rows 16 ti ..) on split fp16, from the fp16 fragments of the log: the same
    // operands, k-slots and order of the MFMAs as the V updates of the 64-wide block pairs (pair64::fused_u, jacobi_vstrip_kernel)
    const half_t* q16 = p.Qr16 + ((size_t)m * npair + h) * (2 * M2 * M2);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = Xs[(16 * ti + li) * PITCH + qfrag16_k<M2>(c, lq, j)];
      half8 bh, bl;
      split_f16x8(x, bh, bl);
      const half8 ah = *reinterpret_cast<const half8*>(q16 + ((size_t)((tj * NCH + c) * 2 + 0) * 64 + lane) * 8);
      const half8 al = *reinterpret_cast<const half8*>(q16 + ((size_t)((tj * NCH + c) * 2 + 1) * 64 + lane) * 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
    }
  } else {
#pragma unroll 4
    for (int kk = 0; kk < M2; kk += 4)      // T = X Qh
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Xs[(16 * ti + li) * PITCH + kk + lq], Qhs[(kk + lq) * PITCH + 16 * tj + li], acc, 0, 0, 0);
  }
  if (!is_v) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) Xs[(16 * ti + 4 * lq + r) * PITCH + 16 * tj + li] = acc[r];
    __syncthreads();
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int kk = 0; kk < M2; kk += 4)      // Y = Qg^T T
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Qgs[(kk + lq) * PITCH + 16 * ti + li], Xs[(kk + lq) * PITCH + 16 * tj + li], acc, 0, 0, 0);
    float* Pw = p.Pw + m * cc;
    const int col = pair_index<B>(16 * tj + li, hi, hj);
#pragma unroll
    for (int r = 0; r < 4; ++r) Pw[(size_t)pair_index<B>(16 * ti + 4 * lq + r, gi, gj) * C + col] = acc[r];
    // mirror tile (h, g): this lane's four rows are four consecutive columns there
    *reinterpret_cast<f32x4*>(Pw + (size_t)col * C + pair_index<B>(16 * ti + 4 * lq, gi, gj)) = acc;
  } else {
    // lane (n, q), register r = (V Qh)[row 16 ti + n][column 16 tj + 4 q + r]: four consecutive columns
    float* Vm = p.V + m * cc;
    *reinterpret_cast<f32x4*>(Vm + (size_t)(g * M2 + 16 * ti + li) * C + pair_index<B>(16 * tj + 4 * lq, hi, hj)) = acc;
  }
}
}  // namespace pair32
