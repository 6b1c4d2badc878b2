// GNBlock with Chain update functions at matrix-core widths: one update function = one kernel (gnx_chain_block_forward_wide, gnx_chain.cpp).
//
//   k_chain_wide<NB, SRC> : a workgroup of 2-4 waves, a wave OWNS 32 rows of the entity through all layers of the function.  The rows live in a
//                           wave-private LDS slice [32][ld] fp32 (ld odd: the A fragments of 32 rows meet in no bank); a Dense layer's 32 x width
//                           output lives in NB (1 or 2) 32 x 32 accumulators, is biased and activated in registers and written back OVER the slice;
//                           a LayerNorm runs row-wise on the slice.  Memory sees the function's input once and its output once.
//
// SRC_EDGE  the lanes gather [ef[e] ; nf[rowval[e]] ; nf[edge_dst[e]] ; gf[graph(e)]] straight into the slice (getedgefninput, gnblock.jl:65; the
//           indices of k_chain_mlp's edge form) — a LayerNorm as the first layer then normalises the gathered row like any other
// SRC_ROWS  a materialised [rows][K] buffer (launch_fn_input: the node and the graph function)
//
// Products: v_mfma_f32_32x32x16_bf16, six terms of the exact three-way split (gnx_x6_mma.h).  The A fragments are split on the fly from the slice
// (x6_frag).  The weights are shared by the workgroup and split ONCE per workgroup, not once per wave: a chunk of 16 reduction steps of the layer's
// [k_in][width] weights goes global -> registers -> three bf16 planes [3][np][16] in LDS (np = the layer's width padded to 32 columns), so a B
// fragment is three 16-byte reads, conflict-free (lane (c, hi) reads bytes 32 c + 16 hi of a plane).  The next chunk's global loads — of this layer
// or of the next Dense — are issued right behind the stores of the current one and land under its matrix instructions (the staging of
// k_ffn_fused).  Every wave walks the same layer and chunk sequence, so the two barriers per chunk are uniform even for a wave whose rows lie
// beyond the entity's end: its rows are zeros at the input and store nothing.  Everything else — input, activations, LayerNorm, output — is
// wave-local and ordered by wave fences alone.
// A last layer of width <= 4 (64 -> 3) runs on the matrix cores as one zero-padded 32-column block like any other: one block of six instructions
// per 16 reduction steps is less than the VALU form's 4 x 64 FMA per row pair, and the kernel keeps one layer path.
// Feature, parameter and output pointers may be 4-byte aligned only: every global access is one dword.  Offsets are size_t.
#include "gnx_chain_mlp.h"  // SRC_*, act helpers
#include "gnx_x6_mma.h"

namespace gnx {

struct ChainWideLayer {
  const float* w;  // Dense: weight [kin][width] / LayerNorm: gamma
  const float* b;  // Dense: bias or nullptr / LayerNorm: beta
  int kin, width;
  int op;          // 0..4: Dense with activation GNX_ACT_*; 5 / 6: LayerNorm with 1 / (sigma + eps) / 1 / sqrt(sigma^2 + eps)
  int next;        // the next Dense layer behind this one, -1: none
};

struct ChainWideArgs {
  ChainWideLayer layer[kChainMaxLayers];
  int n_layers, K, first_dense;
  const float *a0, *a1, *a2;  // EDGE: ef, nf, gf / ROWS: the input rows, -, -
  int d0, d1, d2;
  int N, E, G;
  const int *rowval, *edge_dst, *seg_off;
  float* out; int ow;  // [R][rows][ow]
  size_t rows;
  int ld, waves, bias_off, slice_off;  // ChainWideShape (gnx_chain_plan.h)
};

namespace {
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// two fp32 values (reduction steps 2 kp, 2 kp + 1) -> one dword of each bf16 plane (x6_split8's arithmetic)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = x6_cvt2(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = x6_cvt2(r0, r1);
  l = x6_cvt2(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}
__device__ __forceinline__ x6_bf16x8 plane8(const unsigned* p) { return __builtin_bit_cast(x6_bf16x8, *reinterpret_cast<const x6_u32x4*>(p)); }
}  // namespace

template <int NB, int SRC>
__global__ __launch_bounds__(256) void k_chain_wide(ChainWideArgs a) {
  constexpr int SREG = 2 * NB;  // pairs a thread stages per chunk at 128 threads: 8 * 32 NB / 128
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  unsigned* sW = reinterpret_cast<unsigned*>(s_mem);
  float* sBias = s_mem + a.bias_off;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wv = tid >> 6;
  const int c31 = lane & 31, hi = lane >> 5;
  const int ld = a.ld;
  float* slice = s_mem + a.slice_off + wv * (kChainWideRows * ld);
  const size_t r = blockIdx.y;
  const size_t row0 = ((size_t)blockIdx.x * a.waves + wv) * kChainWideRows;
  const int nrows = row0 >= a.rows ? 0 : (a.rows - row0 < (size_t)kChainWideRows ? (int)(a.rows - row0) : kChainWideRows);

  // ---- the weight staging: cursor (pl, pc) = the chunk the registers hold ----
  float ra[SREG][2], rbias = 0.f;
  int pl = a.first_dense, pc = 0;
  auto load_chunk = [&]() {
    const ChainWideLayer L = a.layer[pl];
    const int npairs = 8 * ceil32(L.width);
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int idx = tid + i * NT, kp = idx & 7, j = idx >> 3, k = 16 * pc + 2 * kp;
      const bool in = idx < npairs && j < L.width;
      ra[i][0] = in && k < L.kin ? L.w[(size_t)k * L.width + j] : 0.f;
      ra[i][1] = in && k + 1 < L.kin ? L.w[(size_t)(k + 1) * L.width + j] : 0.f;
    }
    if (pc == 0) rbias = (tid < L.width && L.b) ? L.b[tid] : 0.f;
  };
  auto store_chunk = [&](int np, bool first) {
#pragma unroll
    for (int i = 0; i < SREG; ++i) {
      const int idx = tid + i * NT;
      if (idx < 8 * np) {
        unsigned h, m, l;
        split2(ra[i][0], ra[i][1], h, m, l);
        sW[idx] = h; sW[8 * np + idx] = m; sW[16 * np + idx] = l;  // plane p, column j, pair kp at (p np + j) 8 + kp; idx = 8 j + kp
      }
    }
    if (first && tid < np) sBias[tid] = rbias;
  };
  if (pl >= 0) load_chunk();

  // ---- the function's input rows into the slice, zero beyond K (to a multiple of 16) and beyond the wave's rows ----
  const int KP = ceil16(a.K);
  {
    int src = 0, dst = 0, g = 0;
    if constexpr (SRC == SRC_EDGE) {
      if (c31 < nrows) {
        const int e = (int)row0 + c31;
        if (a.d1 > 0) { src = a.rowval[e]; dst = a.edge_dst[e]; }
        if (a.d2 > 0) g = segment_of(a.seg_off, a.G, e);
      }
    }
    const int sub = lane >> 4, c16 = lane & 15;
#pragma unroll 1
    for (int r4 = 0; r4 < kChainWideRows / 4; ++r4) {
      const int row = 4 * r4 + sub;
      const int s_ = __shfl(src, row), d_ = __shfl(dst, row), g_ = __shfl(g, row);
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
        slice[row * ld + col] = v;
      }
    }
  }
  wave_sync();

#pragma unroll 1
  for (int l = 0; l < a.n_layers; ++l) {
    const ChainWideLayer L = a.layer[l];
    if (L.op >= 5) {
      // k_chain_layernorm's formula (gnx_chain.cpp): two lanes per row, statistics in registers
      const int d = L.width, half = lane & 1;
      float* xr = slice + (lane >> 1) * ld;
      float s = 0.f;
      for (int k = half; k < d; k += 2) s += xr[k];
      s += __shfl_xor(s, 1);
      const float mu = s / (float)d;
      float v = 0.f;
      for (int k = half; k < d; k += 2) { const float c = xr[k] - mu; v = fmaf(c, c, v); }
      v += __shfl_xor(v, 1);
      v /= (float)d;
      const float inv = L.op == 5 ? 1.f / (sqrtf(v) + kChainLnEps) : 1.f / sqrtf(v + kChainLnEps);
      for (int k = half; k < d; k += 2) xr[k] = fmaf(L.w[k], (xr[k] - mu) * inv, L.b[k]);
      wave_sync();
      continue;
    }
    const int np = ceil32(L.width), nbl = np >> 5, nchunks = ceil16(L.kin) >> 4;
    x6_f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;
#pragma unroll 1
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();  // the readers of the previous chunk (and of the previous layer's bias row) are done
      store_chunk(np, c == 0);
      if (++pc == nchunks) { pl = L.next; pc = 0; }
      if (pl >= 0) load_chunk();  // lands under the matrix instructions below
      __syncthreads();
      const X6Frag fa = x6_frag(slice + c31 * ld + 16 * c + 8 * hi, 1);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < nbl) {
          const unsigned* pb = sW + (32 * b + c31) * 8 + 4 * hi;
          X6Frag fb;
          fb.h = plane8(pb); fb.m = plane8(pb + 8 * np); fb.l = plane8(pb + 16 * np);
          acc[b] = x6_mma(fa, fb, acc[b]);
        }
      }
    }
    // bias, activation, back over the slice: columns up to the next layer's 16-padded reduction width, exactly 0 from `width` on
    wave_sync();
    const int wp = ceil16(L.width);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < nbl) {
        const int col = 32 * b + c31;
        const float bias = sBias[col];
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = acc[b][q] + bias;
        switch (L.op) {  // ONE wave-uniform switch, the loop inside each case
          case 0: break;
          case 1:
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = fmaxf(v[q], 0.f);
            break;
          default:
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = act_apply(v[q], L.op);
            break;
        }
        if (col < wp) {
#pragma unroll
          for (int q = 0; q < 16; ++q) slice[((q & 3) + 8 * (q >> 2) + 4 * hi) * ld + col] = col < L.width ? v[q] : 0.f;
        }
      }
    }
    wave_sync();
  }

  // ---- the wave's rows are one contiguous run of the output: flat, coalesced, each element once ----
  const int n = nrows * a.ow;
  float* __restrict__ o = a.out + (r * a.rows + row0) * (size_t)a.ow;
  for (int i = lane; i < n; i += 64) {
    const int row = i / a.ow;
    o[i] = slice[row * ld + (i - row * a.ow)];
  }
}

// One update function of a Chain block in one launch.  entity 0: in0 / in1 / in2 = ef, nf, gf of widths d0, d1, d2 (SRC_EDGE); 1, 2: in0 = the
// materialised [R rows][d0] input rows (SRC_ROWS; d1 = d2 = 0).  The caller asked chain_wide_takes (gnx_chain_plan.h).
int32_t launch_chain_wide(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                          float* out, int64_t R, hipStream_t s, const char* name) {
  const int K = entity == 0 ? d0 + 2 * d1 + d2 : d0;
  const size_t rows = entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G);
  if (!chain_wide_takes(c, K, rows)) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wide: the function is outside the wide rule");
  if (entity == 0) { if (int32_t rcw = gnx_ensure_wide_tables(h, s)) return rcw; }  // (the destination of every edge)
  const ChainWideShape sh = chain_wide_shape(c, K, rows);
  ChainWideArgs a{};
  int kin = K, last_dense = -1;
  a.first_dense = -1;
  for (int i = 0; i < c.n_layers; ++i) {
    const gnx_dense& l = c.layers[i];
    const bool ln = chain_layer_is_ln(l);
    if (!ln && !l.weight) return fail(GNX_ERR_INVALID_ARG, "Chain: Dense weight is NULL");
    a.layer[i] = ChainWideLayer{l.weight, l.bias, kin, c.widths[i], ln ? 5 + chain_layer_ln_mode(l) : l.act, -1};
    if (!ln) {
      if (last_dense >= 0) a.layer[last_dense].next = i; else a.first_dense = i;
      last_dense = i;
    }
    kin = c.widths[i];
  }
  a.n_layers = c.n_layers; a.K = K;
  a.a0 = in0; a.a1 = in1; a.a2 = in2; a.d0 = d0; a.d1 = d1; a.d2 = d2;
  a.N = (int)h->N; a.E = (int)h->E; a.G = (int)h->G;
  a.rowval = h->d_rowval; a.edge_dst = h->d_edge_dst; a.seg_off = h->d_edge_off;
  a.out = out; a.ow = c.widths[c.n_layers - 1]; a.rows = rows;
  a.ld = sh.ld; a.waves = sh.waves; a.bias_off = sh.bias_off; a.slice_off = sh.slice_off;
  const dim3 grid((unsigned)sh.nwg, (unsigned)R), block(64u * sh.waves);
  const size_t lds = sizeof(float) * (size_t)sh.floats;
  ProfScope ps(name, s);
  auto go = [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (entity == 0) GNX_LAUNCH((k_chain_wide<NB, SRC_EDGE>), grid, block, lds, s, a);
    else GNX_LAUNCH((k_chain_wide<NB, SRC_ROWS>), grid, block, lds, s, a);
  };
  sh.nb == 1 ? go(ChainInt<1>{}) : go(ChainInt<2>{});  // (chain_wide_cut: no function with more blocks is inside the rule)
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
