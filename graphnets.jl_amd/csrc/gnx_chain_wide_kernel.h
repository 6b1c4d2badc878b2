// The text of the Chain forward at matrix-core widths, compiled twice: k_chain_wide (gnx_chain_wide.hip, fp32 features) and k_chain_wide_bf16
// (gnx_chain_wide_bf16.hip, bf16 features).  The work split, the LDS plan (ChainWideShape, gnx_chain_plan.h), the weight staging, LayerNorm, bias
// and activation and the layer loop are one text, so the two kernels cannot drift; with BF = false the text is k_chain_wide as it was written.
//
// A workgroup of 2-4 waves, a wave OWNS 32 rows of the entity through all layers of the function.  The rows live in a wave-private LDS slice
// [32][ld] fp32 (ld odd: the A fragments of 32 rows meet in no bank); a Dense layer's 32 x width output lives in NB (1 or 2) 32 x 32
// accumulators, is biased and activated in registers and written back OVER the slice; a LayerNorm runs row-wise on the slice.
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
//
// BF = true, SRC_EDGE (the bf16 twin's edge form):
//   the gather   ef[e], nf[rowval[e]], nf[edge_dst[e]] and gf[graph(e)] are bf16, the buffers 4-byte aligned.  A lane takes a PAIR of columns
//                of the row: where the two elements are neighbours in memory at a dword boundary they are one dword load, at a segment's odd
//                ends two 16-bit loads — a loaded dword holds two elements of the row, so none straddles the end of a tensor.
//   the row      stays bf16 in LDS where the function opens with a Dense: rows of `chain_wide_bf16_stride(K)` bf16 elements in the memory of the
//                wave's fp32 slice (32 (KP + 8) 2 bytes <= 32 ld 4 bytes for every KP >= 16).  Stride KP + 8 elements = 16 (2 j + 1) bytes: a lane's A
//                fragment — 8 consecutive reduction steps of row c31 at 16 c + 8 hi — is ONE aligned 16-byte read, and the sixteen lanes a 16-byte
//                read serves per pass (consecutive lanes, one `hi`) fall on sixteen different 16-byte columns of the 64 banks.
//   first Dense  the bf16 row is its own high plane, its middle and low planes are exactly zero: the products a.h b.l, a.h b.m, a.h b.h in
//                x6_mma's order with the three all-zero instructions left out — no fragment split, half the matrix instructions, the same bits
//                (an all-zero instruction adds +-0 to an accumulator that started at +0).  The slice is overwritten by the layer's fp32 output only
//                after its last chunk is read, as in the fp32 form; every later Dense is six-term on the fp32 slice.
//   LayerNorm first  the gathered elements are widened (exactly) on their way into the fp32 slice and the kernel proceeds as k_chain_wide.
// BF = true, SRC_ROWS: the materialised fp32 input rows, as k_chain_wide.
// BF = true, output: a wave's rows are one contiguous run of nrows * ow elements: rounded once (to nearest even, x6_cvt2's conversion), stored as
//                dwords with 16-bit odd ends (chain_wave_store_run's way, gnx_chain_wave_bf16.hip); out32: the same rows unrounded for a later
//                function of the call.
// Feature, parameter and output pointers may be 4-byte aligned only.  Offsets are size_t.
#pragma once
#include "gnx_chain_mlp.h"  // SRC_*, act helpers, bf16_t
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
  const float *a0, *a1, *a2;  // EDGE: ef, nf, gf (bf16 in k_chain_wide_bf16, declared float like the feature pointers of BlockArgs) / ROWS: the input rows, -, -
  int d0, d1, d2;
  int N, E, G;
  const int *rowval, *edge_dst, *seg_off;
  float* out; int ow;  // [R][rows][ow] (k_chain_wide_bf16: unused, its outputs follow the record)
  size_t rows;
  int ld, waves, bias_off, slice_off;  // ChainWideShape (gnx_chain_plan.h)
};

__device__ __forceinline__ void chain_wide_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// two fp32 values (reduction steps 2 kp, 2 kp + 1) -> one dword of each bf16 plane (x6_split8's arithmetic)
__device__ __forceinline__ void chain_wide_split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = x6_cvt2(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = x6_cvt2(r0, r1);
  l = x6_cvt2(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}
__device__ __forceinline__ x6_bf16x8 chain_wide_plane8(const unsigned* p) { return __builtin_bit_cast(x6_bf16x8, *reinterpret_cast<const x6_u32x4*>(p)); }

struct ChainWideBf16Args {
  ChainWideArgs f;  // f.a0 .. f.a2: bf16 in the edge form (declared float); f.out unused
  bf16_t* out;      // [R][rows][ow] bf16
  float* out32;     // [R][rows][ow] fp32, or nullptr
};

// The kernel.  The including file defines GNX_CHAIN_WIDE_BF16 as 0 (k_chain_wide) or 1 (k_chain_wide_bf16): the text below is the kernel itself,
// not a function both call — as a kernel's own text k_chain_wide keeps its registers (profiles/chain_wide_resources.json; through a wrapper
// function the same text took 6 VGPRs more).  BF = false: the output is a.out.  BF = true: out_b the bf16 rows, out32 the same rows in fp32 or nullptr.
// k_chain_wide_bf16 is held to three waves per SIMD (amdgpu_waves_per_eu): left alone its two-block edge form took 140 VGPRs + 32 AGPRs — two
// waves per SIMD against k_chain_wide's three — and on the 512-graph 1M-edge batch the call took 0.500 ms against the parent's 0.429; held to 168
// registers (no scratch: profiles/chain_wide_bf16_resources.json) it takes 0.372 (profiles/chain_wide_bf16.json).
#ifndef GNX_CHAIN_WIDE_BF16
#error "define GNX_CHAIN_WIDE_BF16 as 0 or 1 before including gnx_chain_wide_kernel.h"
#endif
template <int NB, int SRC>
#if GNX_CHAIN_WIDE_BF16
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_chain_wide_bf16(ChainWideBf16Args t) {
  constexpr bool BF = true;
  const ChainWideArgs& a = t.f;
  bf16_t* __restrict__ out_b = t.out;
  float* __restrict__ out32 = t.out32;
#else
__global__ __launch_bounds__(256) void k_chain_wide(ChainWideArgs a) {
  constexpr bool BF = false;
  bf16_t* __restrict__ out_b = nullptr;
  float* __restrict__ out32 = nullptr;
#endif
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
        chain_wide_split2(ra[i][0], ra[i][1], h, m, l);
        sW[idx] = h; sW[8 * np + idx] = m; sW[16 * np + idx] = l;  // plane p, column j, pair kp at (p np + j) 8 + kp; idx = 8 j + kp
      }
    }
    if (first && tid < np) sBias[tid] = rbias;
  };
  if (pl >= 0) load_chunk();

  // ---- the function's input rows into the slice, zero beyond K (to a multiple of 16) and beyond the wave's rows ----
  const int KP = ceil16(a.K);
  // (BF) the gathered row stays bf16, at its own stride in the slice's memory, where the first entry is a Dense
  const bool rowbf = BF && SRC == SRC_EDGE && a.layer[0].op < 5;
  const int ldb = chain_wide_bf16_stride(a.K);
  bf16_t* rowb = reinterpret_cast<bf16_t*>(slice);
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
      if constexpr (BF && SRC == SRC_EDGE) {
        // lane c16 of the row's 16 takes the column pairs (2 c16, 2 c16 + 1) + 32 i.  The two elements of a pair are ONE dword load where they
        // are neighbours in memory at an even element (the pair is then inside one tensor's segment: no dword straddles a tensor's end), two
        // 16-bit loads at a segment's odd ends; every load of a row is issued before the first LDS store waits for one.  The pair goes into the
        // bf16 row as one dword, or widened into the fp32 slice.
        auto at = [&](int col) -> const bf16_t* {
          if (col < a.d0) return reinterpret_cast<const bf16_t*>(a.a0) + (r * (size_t)a.E + e) * a.d0 + col;
          if (col < a.d0 + a.d1) return reinterpret_cast<const bf16_t*>(a.a1) + (r * (size_t)a.N + s_) * a.d1 + (col - a.d0);
          if (col < a.d0 + 2 * a.d1) return reinterpret_cast<const bf16_t*>(a.a1) + (r * (size_t)a.N + d_) * a.d1 + (col - a.d0 - a.d1);
          return reinterpret_cast<const bf16_t*>(a.a2) + (r * (size_t)a.G + g_) * a.d2 + (col - a.d0 - 2 * a.d1);
        };
        for (int col = 2 * c16; col < KP; col += 32) {
          unsigned w = 0u;
          if (row < nrows && col < a.K) {
            const bf16_t* __restrict__ p0 = at(col);
            if (col + 1 < a.K) {
              const bf16_t* __restrict__ p1 = at(col + 1);
              const int c1 = col + 1, d01 = a.d0 + a.d1;  // (the same segment: neither of a.d0, d01, d01 + a.d1 lies between the two columns)
              const bool one_seg = c1 != a.d0 && c1 != d01 && c1 != d01 + a.d1;
              if (one_seg && p1 == p0 + 1 && (reinterpret_cast<uintptr_t>(p0) & 3) == 0) w = *reinterpret_cast<const unsigned*>(p0);
              else w = (unsigned)*p0 | ((unsigned)*p1 << 16);
            } else {
              w = *p0;
            }
          }
          if (rowbf) {
            *reinterpret_cast<unsigned*>(rowb + row * ldb + col) = w;
          } else {
            slice[row * ld + col] = __uint_as_float(w << 16);
            slice[row * ld + col + 1] = __uint_as_float(w & 0xffff0000u);
          }
        }
      } else {
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
  }
  chain_wide_sync();

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
      chain_wide_sync();
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
      if (BF && rowbf && l == 0) {  // (BF is a constant; wave-uniform) the bf16 row is the high plane, the other two are zero: three terms, x6_mma's order
        const x6_bf16x8 ah = *reinterpret_cast<const x6_bf16x8*>(rowb + c31 * ldb + 16 * c + 8 * hi);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b < nbl) {
            const unsigned* pb = sW + (32 * b + c31) * 8 + 4 * hi;
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, chain_wide_plane8(pb + 16 * np), acc[b], 0, 0, 0);
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, chain_wide_plane8(pb + 8 * np), acc[b], 0, 0, 0);
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, chain_wide_plane8(pb), acc[b], 0, 0, 0);
          }
        }
        continue;
      }
      const X6Frag fa = x6_frag(slice + c31 * ld + 16 * c + 8 * hi, 1);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < nbl) {
          const unsigned* pb = sW + (32 * b + c31) * 8 + 4 * hi;
          X6Frag fb;
          fb.h = chain_wide_plane8(pb); fb.m = chain_wide_plane8(pb + 8 * np); fb.l = chain_wide_plane8(pb + 16 * np);
          acc[b] = x6_mma(fa, fb, acc[b]);
        }
      }
    }
    // bias, activation, back over the slice: columns up to the next layer's 16-padded reduction width, exactly 0 from `width` on
    chain_wide_sync();
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
    chain_wide_sync();
  }

  // ---- the wave's rows are one contiguous run of the output: flat, coalesced, each element once ----
  const int n = nrows * a.ow;
  if constexpr (BF) {
    if (n <= 0) return;  // wave-uniform, behind the last barrier
    const size_t at = (r * a.rows + row0) * (size_t)a.ow;
    auto el = [&](int j) { const int row = j / a.ow; return slice[row * ld + (j - row * a.ow)]; };
    const int head = (int)(at & 1);
    if (head && lane == 0) out_b[at] = (bf16_t)(x6_cvt2(el(0), 0.f) & 0xffffu);
    const int pairs = (n - head) >> 1;
    unsigned* __restrict__ o32 = reinterpret_cast<unsigned*>(out_b + at + head);
    for (int q = lane; q < pairs; q += 64) {
      const int j = head + 2 * q;
      o32[q] = x6_cvt2(el(j), el(j + 1));
    }
    if (((n - head) & 1) && lane == 63) out_b[at + n - 1] = (bf16_t)(x6_cvt2(el(n - 1), 0.f) & 0xffffu);
    if (out32)
      for (int i = lane; i < n; i += 64) out32[at + i] = el(i);
  } else {
    float* __restrict__ o = a.out + (r * a.rows + row0) * (size_t)a.ow;
    for (int i = lane; i < n; i += 64) {
      const int row = i / a.ow;
      o[i] = slice[row * ld + (i - row * a.ow)];
    }
  }
}

// The record of one update function's launch, shared by launch_chain_wide and launch_chain_wide_bf16.  entity 0: in0 / in1 / in2 = ef, nf, gf of
// widths d0, d1, d2 (SRC_EDGE); 1, 2: in0 = the materialised [R rows][d0] input rows (SRC_ROWS; d1 = d2 = 0).  The caller asked chain_wide_takes.
inline int32_t chain_wide_args(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                               hipStream_t s, const char* who, ChainWideArgs& a, ChainWideShape& sh) {
  const int K = entity == 0 ? d0 + 2 * d1 + d2 : d0;
  const size_t rows = entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G);
  if (!chain_wide_takes(c, K, rows)) return fail(GNX_ERR_INVALID_ARG, std::string(who) + ": the function is outside the wide rule");
  if (entity == 0) { if (int32_t rcw = gnx_ensure_wide_tables(h, s)) return rcw; }  // (the destination of every edge)
  sh = chain_wide_shape(c, K, rows);
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
  a.ow = c.widths[c.n_layers - 1]; a.rows = rows;
  a.ld = sh.ld; a.waves = sh.waves; a.bias_off = sh.bias_off; a.slice_off = sh.slice_off;
  return GNX_OK;
}

}  // namespace gnx
