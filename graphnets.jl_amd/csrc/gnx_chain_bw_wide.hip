// The pullback of one Chain update function at matrix-core widths in one kernel (gnx_chain_block_backward_wide, gnx_backward.hip).
//
//   k_chain_bw_wide<NB, SRC> : a PERSISTENT grid of at most kChainBwWideGrid workgroups per replica, 2-4 waves each; a workgroup loops over tiles
//   of 32 rows per wave.  A wave owns its 32 rows through the whole function: it runs the forward again into a wave-private LDS tape
//   [32][ld] fp32 (ChainBwWideShape, gnx_chain_plan.h: the input row, every entry's output, a gelu Dense's pre-activation, a LayerNorm's
//   (mu, sigma + eps, q); ld odd) and walks back over it.  The delta of entry l is written OVER entry l's output (its act' is read from the
//   very element it replaces; a gelu entry reads its pre-activation), so the tape has no delta slot.  Nothing row-sized reaches memory but the
//   input gradient of the function.
//
// Products, all v_mfma_f32_32x32x16_bf16 over the six-term split (gnx_x6_mma.h), C/D layout row (q & 3) + 8 (q >> 2) + 4 hi, column c:
//   forward  Y = X W       A: the wave's rows, tape row c, 8 consecutive k (stride 1)        B: the staged chunk of W, column j, 16 k
//   dX = D W^T             A: the wave's deltas, tape row c, 8 consecutive j (stride 1)      B: the staged chunk of W^T, column k, 16 j
//   dW = X^T D             A: tape COLUMN k, 8 consecutive rows (stride ld)                  B: tape column j of the deltas, the same 8 rows
// The staged chunk is k_chain_wide's: 16 reduction steps as three bf16 planes [3][32 NB][16], split once per workgroup, the next chunk's global
// loads issued behind the current chunk's stores, under its matrix instructions; W^T is staged by reading W transposed (eight lanes read 16
// consecutive floats of a row of W).  The runs of chunks are a table of the plan (item[]), walked by one cursor across entries and tiles.
//
// Parameter gradients: the 32 x 32 blocks of every dW are dealt to the waves of the workgroup (block b: wave b % waves, register slot
// b / waves, at most kChainBwWideAcc slots); behind a barrier a wave reduces its blocks over ALL of the workgroup's rows, reading every wave's
// tape column-wise.  db, dgamma and dbeta are column sums by the lanes of wave l % waves, four registers per entry.  All accumulators stay in
// registers across the workgroup's tiles; a workgroup writes ONE partial row per entry at its end, in k_bw_dw_final's pair order (p = k J + j,
// k = K the bias; a LayerNorm gamma then beta), so partial rows are bounded by the grid whatever the rows.  No atomics, every order fixed.
// A wave whose rows lie beyond the entity's end walks the same barriers: its input rows and upstream gradients are zeros, so are all its
// deltas — it adds nothing and stores nothing.  Every global access is one dword; offsets are size_t.
#include "gnx_chain_mlp.h"  // SRC_*, act helpers
#include "gnx_x6_mma.h"

namespace gnx {

struct ChainBwWideLayer {
  const float* w;  // Dense: weight [kin][width] / LayerNorm: gamma
  const float* b;  // Dense: bias or nullptr / LayerNorm: beta
  int kin, width;
  int op;          // 0..4: Dense with activation GNX_ACT_*; 5 / 6: LayerNorm with 1 / (sigma + eps) / 1 / sqrt(sigma^2 + eps)
  int in_off, out_off, aux_off, part_off;  // tape slots, the entry's place in a partial row
};

struct ChainBwWideArgs {
  ChainBwWideLayer layer[kChainBwWideMaxLayers];
  unsigned char item[kChainBwWideMaxItems][4];  // entry, transposed, pass, chunks
  unsigned char block[4 * kChainBwWideAcc][3];  // entry, kb, jb
  int n_layers, n_items, n_blocks, K;
  const float *a0, *a1, *a2;  // EDGE: ef, nf, gf / ROWS: the input rows, -, -
  int d0, d1, d2;
  int N, E, G;
  const int *rowval, *edge_dst, *seg_off;  // seg_off: the entity's rows by graph (edges: d_edge_off, nodes: d_node_off)
  size_t rows, ntiles;
  int ld, waves, bias_off, tape_off;
  const float* Gup;                                           // upstream gradient [R][rows][ow] or nullptr
  const float* ex1; int ex1_stride, ex1_off; size_t ex1_rep;  // dXg rows by graph, or nullptr
  const float* ex2; int ex2_stride; size_t ex2_rep;           // EDGE: dXn rows by destination node, or nullptr
  float* dx; int dx_c0;                                       // columns [dx_c0, K) of the input gradient, or nullptr
  float* direct;                                              // columns [0, dx_c0), or nullptr
  float* part;                                                // partial rows, entry l at part + part_off[l] * (R nwg); or nullptr
};

namespace {
__device__ __forceinline__ void bww_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// two fp32 values (reduction steps 2 kp, 2 kp + 1) -> one dword of each bf16 plane (x6_split8's arithmetic)
__device__ __forceinline__ void bww_split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = x6_cvt2(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = x6_cvt2(r0, r1);
  l = x6_cvt2(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}
__device__ __forceinline__ x6_bf16x8 bww_plane8(const unsigned* p) { return __builtin_bit_cast(x6_bf16x8, *reinterpret_cast<const x6_u32x4*>(p)); }
__device__ __forceinline__ int bww_row(int q, int hi) { return (q & 3) + 8 * (q >> 2) + 4 * hi; }  // the C/D layout's row of element q
}  // namespace

template <int NB, int SRC>
__global__ __launch_bounds__(256) void k_chain_bw_wide(ChainBwWideArgs a) {
  constexpr int SREG = 2 * NB;   // pairs a thread stages per chunk at 128 threads: 8 * 32 NB / 128
  constexpr int NP = 32 * NB;    // columns of the staged chunk
  constexpr int ACC = kChainBwWideAcc, ML = kChainBwWideMaxLayers, ROWS = kChainWideRows;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  unsigned* sW = reinterpret_cast<unsigned*>(s_mem);
  float* sBias = s_mem + a.bias_off;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c31 = lane & 31, hi = lane >> 5;
  const int ld = a.ld, nl = a.n_layers, waves = a.waves;
  float* const tapes = s_mem + a.tape_off;
  float* const tape = tapes + wv * (ROWS * ld);
  const size_t r = blockIdx.y;
  const bool want_gin0 = a.dx || a.direct;

  // ---- the parameter-gradient accumulators: registers across the workgroup's tiles ----
  x6_f32x16 dw[ACC];
#pragma unroll
  for (int s = 0; s < ACC; ++s)
#pragma unroll
    for (int q = 0; q < 16; ++q) dw[s][q] = 0.f;
  float v0[ML], v1[ML], v2[ML], v3[ML];  // Dense: v0 = db[lane]; LayerNorm: dgamma[lane], dgamma[lane + 64], dbeta[lane], dbeta[lane + 64]
#pragma unroll
  for (int l = 0; l < ML; ++l) v0[l] = v1[l] = v2[l] = v3[l] = 0.f;

  for (int i = lane; i < ROWS * ld; i += 64) tape[i] = 0.f;  // (slack and padding: finite from the start)

  // ---- the weight staging: cursor (si, pc) = the chunk the registers hold; -1: none ----
  float ra[SREG][2], rbias = 0.f;
  int si = a.n_items > 0 ? 0 : -1, pc = 0;
  auto load_chunk = [&]() {
    const int li = a.item[si][0], T = a.item[si][1], c0 = NP * a.item[si][2];
    const ChainBwWideLayer& L = a.layer[li];
    const float* __restrict__ w = L.w;
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int idx = tid + i * NT, kp = idx & 7, col = c0 + (idx >> 3), red = 16 * pc + 2 * kp;
      const bool in = idx < 8 * NP;
      if (T) {  // W^T: column = input index k, reduction = output index j
        const bool ok = in && col < L.kin;
        ra[i][0] = ok && red < L.width ? w[(size_t)col * L.width + red] : 0.f;
        ra[i][1] = ok && red + 1 < L.width ? w[(size_t)col * L.width + red + 1] : 0.f;
      } else {
        const bool ok = in && col < L.width;
        ra[i][0] = ok && red < L.kin ? w[(size_t)red * L.width + col] : 0.f;
        ra[i][1] = ok && red + 1 < L.kin ? w[(size_t)(red + 1) * L.width + col] : 0.f;
      }
    }
    if (!T && pc == 0) rbias = (tid < L.width && L.b) ? L.b[tid] : 0.f;
  };
  auto store_chunk = [&](bool bias) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int idx = tid + i * NT;
      if (idx < 8 * NP) {
        unsigned h, m, l;
        bww_split2(ra[i][0], ra[i][1], h, m, l);
        sW[idx] = h; sW[8 * NP + idx] = m; sW[16 * NP + idx] = l;  // plane p, column j, pair kp at (p NP + j) 8 + kp; idx = 8 j + kp
      }
    }
    if (bias && tid < NP) sBias[tid] = rbias;
  };
  if (si >= 0) load_chunk();

#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool more = tile + gridDim.x < a.ntiles;
    // one step of the cursor, and the next chunk's loads (they land under the matrix instructions that follow)
    auto advance = [&]() {
      if (++pc == a.item[si][3]) {
        pc = 0;
        if (++si == a.n_items) si = more ? 0 : -1;
      }
      if (si >= 0) load_chunk();
    };
    __syncthreads();  // the previous tile's readers of this wave's tape are done
    const size_t row0 = (tile * waves + wv) * ROWS;
    const int nrows = row0 >= a.rows ? 0 : (a.rows - row0 < (size_t)ROWS ? (int)(a.rows - row0) : ROWS);

    // ---- the function's input rows onto the tape, zero beyond K (to a multiple of 16) and beyond the wave's rows ----
    int g_row = 0, dst_row = 0;  // lane c31: the graph and (EDGE) the destination node of row c31
    {
      const int KP = ceil16(a.K);
      int src = 0;
      if (c31 < nrows) {
        const int e = (int)row0 + c31;
        if constexpr (SRC == SRC_EDGE) {
          if (a.d1 > 0 || a.ex2) dst_row = a.edge_dst[e];
          if (a.d1 > 0) src = a.rowval[e];
          if (a.d2 > 0 || a.ex1) g_row = segment_of(a.seg_off, a.G, e);
        } else {
          if (a.ex1) g_row = segment_of(a.seg_off, a.G, e);
        }
      }
      const int sub = lane >> 4, c16 = lane & 15;
#pragma unroll 1
      for (int r4 = 0; r4 < ROWS / 4; ++r4) {
        const int row = 4 * r4 + sub;
        const int s_ = __shfl(src, row), d_ = __shfl(dst_row, row), g_ = __shfl(g_row, row);
        const size_t e = row0 + row;
        for (int col = c16; col < KP; col += 16) {
          float v = 0.f;
          if (row < nrows && col < a.K) {
            if constexpr (SRC == SRC_EDGE) {
              if (col < a.d0) v = a.a0[(r * (size_t)a.E + e) * a.d0 + col];
              else if (col < a.d0 + a.d1) v = a.a1[(r * (size_t)a.N + s_) * a.d1 + (col - a.d0)];
              else if (col < a.d0 + 2 * a.d1) v = a.a1[(r * (size_t)a.N + d_) * a.d1 + (col - a.d0 - a.d1)];
              else v = a.a2[(r * (size_t)a.G + g_) * a.d2 + (col - a.d0 - 2 * a.d1)];
            } else {
              v = a.a0[(r * a.rows + e) * (size_t)a.K + col];
            }
          }
          tape[row * ld + col] = v;
        }
      }
    }
    bww_wave_sync();

    // ---- forward: every entry's output into its slot ----
#pragma unroll 1
    for (int l = 0; l < nl; ++l) {
      const ChainBwWideLayer L = a.layer[l];
      if (L.op >= 5) {
        // k_chain_wide's LayerNorm: two lanes per row; the row's statistics stay on the tape for the way back
        const int d = L.width, half = lane & 1, dp = ceil16(d);
        const float* xr = tape + (lane >> 1) * ld + L.in_off;
        float* yr = tape + (lane >> 1) * ld + L.out_off;
        float s = 0.f;
        for (int k = half; k < d; k += 2) s += xr[k];
        s += __shfl_xor(s, 1);
        const float mu = s / (float)d;
        float v = 0.f;
        for (int k = half; k < d; k += 2) { const float c = xr[k] - mu; v = fmaf(c, c, v); }
        v += __shfl_xor(v, 1);
        v /= (float)d;
        const float sigma = sqrtf(v);
        const float sden = L.op == 5 ? sigma + kChainLnEps : sqrtf(v + kChainLnEps);
        const float inv = 1.f / sden;
        for (int k = half; k < dp; k += 2) yr[k] = k < d ? fmaf(L.w[k], (xr[k] - mu) * inv, L.b[k]) : 0.f;
        if (half == 0) {
          float* st = tape + (lane >> 1) * ld + L.aux_off;
          st[0] = mu; st[1] = sden; st[2] = L.op == 5 ? sigma * sden * sden : sden * sden * sden;
        }
        bww_wave_sync();
        continue;
      }
      const int nbl = ceil32(L.width) >> 5, nchunks = ceil16(L.kin) >> 4;
      x6_f32x16 acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;
#pragma unroll 1
      for (int c = 0; c < nchunks; ++c) {
        __syncthreads();  // the readers of the previous chunk (and of the previous entry's bias row) are done
        store_chunk(c == 0);
        advance();
        __syncthreads();
        const X6Frag fa = x6_frag(tape + c31 * ld + L.in_off + 16 * c + 8 * hi, 1);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b < nbl) {
            const unsigned* pb = sW + (32 * b + c31) * 8 + 4 * hi;
            X6Frag fb;
            fb.h = bww_plane8(pb); fb.m = bww_plane8(pb + 8 * NP); fb.l = bww_plane8(pb + 16 * NP);
            acc[b] = x6_mma(fa, fb, acc[b]);
          }
        }
      }
      // bias, activation, into the entry's slot: exactly 0 from `width` to the 16-padded width; a gelu entry keeps its pre-activation too
      const int wp = ceil16(L.width);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < nbl) {
          const int col = 32 * b + c31;
          const float bias = sBias[col];
          if (col < wp) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const float z = col < L.width ? acc[b][q] + bias : 0.f;
              float* const at = tape + bww_row(q, hi) * ld + col;
              if (L.op == GNX_ACT_GELU) at[L.aux_off] = z;
              at[L.out_off] = col < L.width ? (L.op == 1 ? fmaxf(z, 0.f) : act_apply(z, L.op)) : 0.f;
            }
          }
        }
      }
      bww_wave_sync();
    }

    // ---- delta of the last entry over its output: (upstream + the shares of the levels above) .* act' ----
    {
      const ChainBwWideLayer L = a.layer[nl - 1];
      const int ow = L.width, owp = ceil16(ow), act = L.op < 5 ? L.op : GNX_ACT_IDENTITY;
      const int ysrc = L.op == GNX_ACT_GELU ? L.aux_off : L.out_off;
#pragma unroll 1
      for (int i0 = 0; i0 < ROWS * owp; i0 += 64) {
        const int i = i0 + lane, row = i / owp, k = i - row * owp;  // (32 owp is a multiple of 64: row < 32 for every lane)
        const int g_ = __shfl(g_row, row), d_ = __shfl(dst_row, row);
        float v = 0.f;
        if (row < nrows && k < ow) {
          float g = a.Gup ? a.Gup[(r * a.rows + row0 + row) * (size_t)ow + k] : 0.f;
          if (a.ex1) g += a.ex1[r * a.ex1_rep + (size_t)g_ * a.ex1_stride + a.ex1_off + k];
          if constexpr (SRC == SRC_EDGE) {
            if (a.ex2) g += a.ex2[r * a.ex2_rep + (size_t)d_ * a.ex2_stride + k];
          }
          v = g * act_grad_bw(tape[row * ld + ysrc + k], act);
        }
        tape[row * ld + L.out_off + k] = v;
      }
    }

    // ---- back through the entries ----
#pragma unroll 1
    for (int l = nl - 1; l >= 0; --l) {
      const ChainBwWideLayer L = a.layer[l];
      const bool want_gin = l > 0 || want_gin0;
      const int pop = l > 0 ? a.layer[l - 1].op : 0;                 // the entry in front: its act' makes its delta from this entry's dX
      const int pact = l > 0 && pop >= 1 && pop <= 4 ? pop : 0;      // (identity and LayerNorm: the gradient as it stands)
      const int psrc = pact == GNX_ACT_GELU ? a.layer[l - 1].aux_off : L.in_off;
      __syncthreads();  // every wave's delta of this entry is in place
      if (L.op >= 5) {
        // k_ln_backward with one norm: dx = (dxh - mean(dxh)) / sden - c * coef, dxh = dy .* gamma; two lanes per row
        const int d = L.width, half = lane & 1, rowi = lane >> 1;
        float* xr = tape + rowi * ld + L.in_off;
        const float* dy = tape + rowi * ld + L.out_off;
        const float* st = tape + rowi * ld + L.aux_off;
        const float mu = st[0], sden = st[1], qq = st[2];
        float sum_dxh = 0.f, sum_dxh_c = 0.f;
        for (int k = half; k < d; k += 2) {
          const float dxh = dy[k] * L.w[k];
          sum_dxh += dxh;
          sum_dxh_c = fmaf(dxh, xr[k] - mu, sum_dxh_c);
        }
        sum_dxh += __shfl_xor(sum_dxh, 1);
        sum_dxh_c += __shfl_xor(sum_dxh_c, 1);
        if (a.part && wv == l % waves) {  // dgamma = column sums of dy .* xhat, dbeta = of dy, over all of the workgroup's rows in row order
          float sg0 = 0.f, sg1 = 0.f, sb0 = 0.f, sb1 = 0.f;
          const int j0 = lane < d ? lane : 0, j1 = lane + 64 < d ? lane + 64 : 0;
#pragma unroll 1
          for (int i = 0; i < waves * ROWS; ++i) {
            const float* t = tapes + i * ld;
            const float m_ = t[L.aux_off], sd = t[L.aux_off + 1];
            const float y0 = t[L.out_off + j0], y1 = t[L.out_off + j1];
            sb0 += y0; sb1 += y1;
            sg0 = fmaf(y0, (t[L.in_off + j0] - m_) / sd, sg0);
            sg1 = fmaf(y1, (t[L.in_off + j1] - m_) / sd, sg1);
          }
#pragma unroll
          for (int u = 0; u < ML; ++u)
            if (u == l) { v0[u] += sg0; v1[u] += sg1; v2[u] += sb0; v3[u] += sb1; }
        }
        if (want_gin) {
          __syncthreads();  // the column sums have read this wave's x and dy
          const float mean_dxh = sum_dxh / (float)d;
          const float coef = qq > 0.f ? sum_dxh_c / ((float)d * qq) : 0.f;
          const bool live = rowi < nrows;
          const size_t at = r * a.rows + row0 + rowi;
          for (int k = half; k < d; k += 2) {
            const float x = xr[k];
            const float gin = (dy[k] * L.w[k] - mean_dxh) / sden - (x - mu) * coef;
            if (l > 0) {
              xr[k] = pact ? gin * act_grad_bw(pact == GNX_ACT_GELU ? tape[rowi * ld + psrc + k] : x, pact) : gin;
            } else if (live) {
              if (k < a.dx_c0) { if (a.direct) a.direct[at * (size_t)a.dx_c0 + k] = gin; }
              else if (a.dx) a.dx[at * (size_t)(a.K - a.dx_c0) + (k - a.dx_c0)] = gin;
            }
          }
        }
        continue;
      }
      if (a.part) {
        // dW = X^T D: this wave's blocks of the entry over every wave's rows, 16 rows per matrix step
#pragma unroll
        for (int s = 0; s < ACC; ++s) {
          const int b = s * waves + wv;
          if (b < a.n_blocks && a.block[b][0] == l) {
            const int xo = L.in_off + 32 * a.block[b][1] + c31, dofs = L.out_off + 32 * a.block[b][2] + c31;
#pragma unroll 1
            for (int i = 0; i < waves * ROWS; i += 16) {
              const float* t = tapes + (i + 8 * hi) * ld;
              const X6Frag fa = x6_frag(t + xo, ld), fb = x6_frag(t + dofs, ld);
              dw[s] = x6_mma(fa, fb, dw[s]);
            }
          }
        }
        if (wv == l % waves) {  // db: column sums of the deltas in row order
          float sb = 0.f;
          const int j = lane < L.width ? lane : 0;
#pragma unroll 1
          for (int i = 0; i < waves * ROWS; ++i) sb += tapes[i * ld + L.out_off + j];
#pragma unroll
          for (int u = 0; u < ML; ++u)
            if (u == l) v0[u] += sb;
        }
      }
      if (!want_gin) continue;
      // dX = D W^T in passes of NP input columns; a pass's result becomes the delta of the entry in front, over that entry's output
      const int nchunks = ceil16(L.width) >> 4, kblocks = ceil32(L.kin) >> 5, kp16 = ceil16(L.kin);
#pragma unroll 1
      for (int pass = 0; pass * NP < L.kin; ++pass) {
        x6_f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;
#pragma unroll 1
        for (int c = 0; c < nchunks; ++c) {
          __syncthreads();  // the readers of the previous chunk are done (first chunk: every wave is through this entry's dW)
          store_chunk(false);
          advance();
          __syncthreads();
          const X6Frag fa = x6_frag(tape + c31 * ld + L.out_off + 16 * c + 8 * hi, 1);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (pass * NB + b < kblocks) {
              const unsigned* pb = sW + (32 * b + c31) * 8 + 4 * hi;
              X6Frag fb;
              fb.h = bww_plane8(pb); fb.m = bww_plane8(pb + 8 * NP); fb.l = bww_plane8(pb + 16 * NP);
              acc[b] = x6_mma(fa, fb, acc[b]);
            }
          }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int col = 32 * (pass * NB + b) + c31;
          if (pass * NB + b < kblocks && col < kp16) {
            if (l > 0) {
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                float* const at = tape + bww_row(q, hi) * ld;
                float v = 0.f;
                if (col < L.kin) v = pact ? acc[b][q] * act_grad_bw(at[psrc + col], pact) : acc[b][q];
                at[L.in_off + col] = v;
              }
            } else if (col < a.K) {
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int row = bww_row(q, hi);
                if (row < nrows) {
                  const size_t at = r * a.rows + row0 + row;
                  if (col < a.dx_c0) { if (a.direct) a.direct[at * (size_t)a.dx_c0 + col] = acc[b][q]; }
                  else if (a.dx) a.dx[at * (size_t)(a.K - a.dx_c0) + (col - a.dx_c0)] = acc[b][q];
                }
              }
            }
          }
        }
      }
    }
  }

  // ---- one partial row per entry and workgroup, straight from the registers ----
  if (!a.part) return;
  const size_t wg = r * gridDim.x + blockIdx.x, nwg = (size_t)gridDim.x * gridDim.y;
#pragma unroll
  for (int s = 0; s < ACC; ++s) {
    const int b = s * waves + wv;
    if (b < a.n_blocks) {
      const ChainBwWideLayer& L = a.layer[a.block[b][0]];
      float* __restrict__ out = a.part + (size_t)L.part_off * nwg + wg * (size_t)(L.width * (L.kin + 1));
      const int j = 32 * a.block[b][2] + c31;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int k = 32 * a.block[b][1] + bww_row(q, hi);
        if (k < L.kin && j < L.width) out[(size_t)k * L.width + j] = dw[s][q];
      }
    }
  }
#pragma unroll
  for (int l = 0; l < ML; ++l) {
    if (l < nl && wv == l % waves) {
      const ChainBwWideLayer& L = a.layer[l];
      const int J = L.width;
      if (L.op < 5) {
        float* __restrict__ out = a.part + (size_t)L.part_off * nwg + wg * (size_t)(J * (L.kin + 1)) + (size_t)L.kin * J;
        if (lane < J) out[lane] = v0[l];
      } else {
        float* __restrict__ out = a.part + (size_t)L.part_off * nwg + wg * (size_t)(2 * J);
        if (lane < J) { out[lane] = v0[l]; out[J + lane] = v2[l]; }
        if (lane + 64 < J) { out[lane + 64] = v1[l]; out[J + lane + 64] = v3[l]; }
      }
    }
  }
}

// The pullback of one update function in one launch.  entity 0: in0 / in1 / in2 = ef, nf, gf of widths d0, d1, d2 (SRC_EDGE); 1, 2: in0 = the
// materialised [R rows][d0] input rows (SRC_ROWS; d1 = d2 = 0).  io: launch_chain_bw_narrow's contract (the partial rows: chain_bw_wide_shape's P
// and nwg).  The caller asked chain_bw_wide_takes, made sure of the handle's matrix-core tables (the destination of every edge) and opens the
// ProfScope.
int32_t launch_chain_bw_wide(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                             const ChainBwNarrowIo& io, int64_t R, hipStream_t s) {
  const int K = entity == 0 ? d0 + 2 * d1 + d2 : d0;
  const size_t rows = entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G);
  if (!chain_bw_wide_takes(c, K, rows)) return fail(GNX_ERR_INVALID_ARG, "launch_chain_bw_wide: the function is outside the wide pullback's rule");
  const ChainBwWideShape sh = chain_bw_wide_shape(c, K, rows);
  ChainBwWideArgs a{};
  int kin = K;
  for (int i = 0; i < c.n_layers; ++i) {
    const gnx_dense& l = c.layers[i];
    const bool ln = chain_layer_is_ln(l);
    if (!l.weight || (ln && !l.bias)) return fail(GNX_ERR_INVALID_ARG, ln ? "Chain: LayerNorm gamma / beta is NULL" : "Chain: Dense weight is NULL");
    a.layer[i] = ChainBwWideLayer{l.weight, l.bias, kin, c.widths[i], ln ? 5 + chain_layer_ln_mode(l) : l.act, sh.in_off[i], sh.out_off[i], sh.aux_off[i], sh.part_off[i]};
    kin = c.widths[i];
  }
  const bool dx0 = io.dx || io.direct;
  a.n_items = dx0 ? sh.n_items_dx0 : sh.n_items;
  for (int i = 0; i < a.n_items; ++i)
    for (int k = 0; k < 4; ++k) a.item[i][k] = sh.item[i][k];
  a.n_blocks = sh.n_blocks;
  for (int i = 0; i < sh.n_blocks; ++i)
    for (int k = 0; k < 3; ++k) a.block[i][k] = sh.block[i][k];
  a.n_layers = c.n_layers; a.K = K;
  a.a0 = in0; a.a1 = in1; a.a2 = in2; a.d0 = d0; a.d1 = d1; a.d2 = d2;
  a.N = (int)h->N; a.E = (int)h->E; a.G = (int)h->G;
  a.rowval = h->d_rowval; a.edge_dst = h->d_edge_dst; a.seg_off = entity == 1 ? h->d_node_off : h->d_edge_off;
  a.rows = rows; a.ntiles = sh.ntiles;
  a.ld = sh.ld; a.waves = sh.waves; a.bias_off = sh.bias_off; a.tape_off = sh.tape_off;
  a.Gup = io.G;
  a.ex1 = entity < 2 ? io.ex1 : nullptr; a.ex1_stride = io.ex1_stride; a.ex1_off = io.ex1_off; a.ex1_rep = (size_t)h->G * io.ex1_stride;
  a.ex2 = entity == 0 ? io.ex2 : nullptr; a.ex2_stride = io.ex2_stride; a.ex2_rep = (size_t)h->N * io.ex2_stride;
  a.dx = io.dx; a.dx_c0 = io.dx_c0; a.direct = io.direct; a.part = io.part;
  const dim3 grid((unsigned)sh.nwg, (unsigned)R), block(64u * sh.waves);
  const size_t lds = sizeof(float) * (size_t)sh.floats;
  auto go = [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (entity == 0) GNX_LAUNCH((k_chain_bw_wide<NB, SRC_EDGE>), grid, block, lds, s, a);
    else GNX_LAUNCH((k_chain_bw_wide<NB, SRC_ROWS>), grid, block, lds, s, a);
  };
  sh.nb == 1 ? go(ChainInt<1>{}) : go(ChainInt<2>{});  // (chain_wide_cut: no function with more blocks is inside the rule)
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
