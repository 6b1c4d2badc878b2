// The wave form of the Chain forward on bfloat16 feature rows (gnx_chain_block_forward_wave_typed, gnx_chain.cpp; the rule:
// chain_wave_typed_takes, gnx_chain_plan.h).
//
//   k_chain_wave_bf16<W>       : k_chain_wave (gnx_chain_wave.hip) — one wavefront per wave tile, both functions' parameters staged once per
//                                workgroup, the layers run by chain_layer_fw, the node sums in CSC order and the partial row's wave_sum trees,
//                                all of it operation for operation — with another way for the data in and out:
//     loads                      ef, nf[src], nf[dst], nf[n] and gf[g] are bf16: one 16-bit load per element, widened exactly
//                                (chain_load_seg_bf16); nothing beyond 2-byte alignment of a row is assumed.
//     lanes as EDGES             the finished row goes to the wave's LDS slice [cap][oe | 1] as unrounded fp32 and nowhere else: the node sums and
//                                the partial row's edge half read the fp32 kernel's bits.
//     the ef' store              a tile's ef' is ONE contiguous run of ne * oe bf16 elements from element (r E + e0) oe of the output.  Behind
//                                the fence the wave stores the run flat (chain_wave_store_run): lane l takes the dwords l, l + 64, ... of the
//                                run, reads the two elements of a dword from the slice, rounds each once (to nearest even) and stores the pair;
//                                a run that starts or ends on an odd element has that one element stored as 16 bits.  The buffer is 4-byte
//                                aligned (the entry checks), so an even element index is a dword boundary; no byte outside the run is touched.
//     lanes as NODES             as k_chain_wave; then, behind a wavefront fence (every lane has summed its in-edges' rows), the wave writes its
//                                nn rows over the slice at row stride on | 1 and stores them as the run of nn * on elements from (r N + n0) on.
//                                The slice therefore holds max(cap (oe | 1), 64 (on | 1)) floats.  The node half of the partial row is taken
//                                from registers before that.
//   k_chain_graph_wave_bf16<W> : k_chain_graph_wave with gf read as bf16 and gf' rounded once on the store; the partial rows stay fp32.
//
// Each bf16 output is written exactly once and no fp32 copy of anything E- or N-sized exists: beside the partial rows the call has no workspace.
// Finite data: the three outputs are to_bf16 of k_chain_wave's / k_chain_graph_wave's on the exactly widened inputs, bit for bit.
// Compiled without the packed fp32 instructions, like gnx_chain_wave.hip (build.py).
#include "gnx_chain_mlp.h"

namespace gnx {

struct ChainWaveBf16Args {
  ChainMlpArgs e, n;  // as ChainWaveArgs; e.a0 .. e.a2 and n.a1, n.a2 point at bf16 rows (declared float, like the feature pointers of BlockArgs)
  const Tile* wtiles;
  int n_wtiles, waves, slice;        // waves per workgroup; floats of a wave's LDS slice: max(cap (oe | 1), 64 (on | 1))
  int par_e, par_all;                // floats of the edge function's / of both functions' staged parameters
  bf16_t *ef_out, *nf_out;
  float* partials;                   // [R][n_wtiles][oe + on], or nullptr (no graph function)
  int oe, on;
  unsigned inv_oe, inv_on;           // chain_wave_inv of oe / on
};

// Rows of width d at row stride d | 1: flat element j = row * d + col sits at float j + row of the slice for an even d (stride d + 1) and at j
// for an odd one.  row = j / d as one multiply-high: with m = 2^32 / d + 1 (d even, so m fits), j m / 2^32 = j / d + j e / (d 2^32), 0 < e <= d, and
// a slice has fewer than 2^14 elements.  An odd d: m = 0.
inline unsigned chain_wave_inv(int d) { return (d & 1) ? 0u : (unsigned)(0x100000000ull / (unsigned)d) + 1u; }

// The wave's rows in its slice `s` as one run of L bf16 elements from element `at` of `out`: dwords across the lanes, the run's odd ends as single
// 16-bit stores.
__device__ __forceinline__ void chain_wave_store_run(const float* __restrict__ s, unsigned inv, bf16_t* __restrict__ out, size_t at, int L, int lane) {
  if (L <= 0) return;  // wave-uniform
  auto el = [&](int j) { return s[j + (int)__umulhi((unsigned)j, inv)]; };
  const int head = (int)(at & 1);
  if (head && lane == 0) out[at] = to_bf16(el(0));
  const int pairs = (L - head) >> 1;
  unsigned* __restrict__ o32 = reinterpret_cast<unsigned*>(out + at + head);
  for (int q = lane; q < pairs; q += 64) {
    const int j = head + 2 * q;
    o32[q] = pack_bf16(el(j), el(j + 1));
  }
  if (((L - head) & 1) && lane == 63) out[at + L - 1] = to_bf16(el(L - 1));
}

template <int W>
__global__ __launch_bounds__(256) void k_chain_wave_bf16(ChainWaveBf16Args a) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int NT = 64 * a.waves;
  chain_stage_params(a.e, s_mem, NT);
  chain_stage_params(a.n, s_mem + a.par_e, NT);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wt = blockIdx.x * a.waves + wave;
  if (wt >= a.n_wtiles) return;  // wave-uniform
  const size_t r = blockIdx.y;
  const Tile t = a.wtiles[wt];
  const int ne = t.e1 - t.e0, nn = t.n1 - t.n0, oe = a.oe, on = a.on, se = oe | 1, sn = on | 1;
  float* __restrict__ s_row = s_mem + a.par_all + wave * a.slice;
  const bf16_t* __restrict__ ef = reinterpret_cast<const bf16_t*>(a.e.a0);
  const bf16_t* __restrict__ nf = reinterpret_cast<const bf16_t*>(a.e.a1);
  const bf16_t* __restrict__ gfr = reinterpret_cast<const bf16_t*>(a.e.a2) + (r * (size_t)a.e.G + t.g) * a.e.d2;

  // ---- lanes as edges ----
  for (int base = 0; base < ne; base += 64) {  // (wave-uniform trips: every lane runs the layers, a lane beyond the tile on a zero row)
    const int el = base + lane;
    const bool live = el < ne;
    float cur[W];
#pragma unroll
    for (int k = 0; k < W; ++k) cur[k] = 0.f;
    if (live) {
      const int e = t.e0 + el;
      if (a.e.d0 > 0) chain_load_seg_bf16<W>(ef + (r * (size_t)a.e.E + e) * a.e.d0, 0, a.e.d0, cur);
      if (a.e.d1 > 0) {
        chain_load_seg_bf16<W>(nf + (r * (size_t)a.e.N + a.e.rowval[e]) * a.e.d1, a.e.d0, a.e.d1, cur);
        chain_load_seg_bf16<W>(nf + (r * (size_t)a.e.N + a.e.edge_dst[e]) * a.e.d1, a.e.d0 + a.e.d1, a.e.d1, cur);
      }
      if (a.e.d2 > 0) chain_load_seg_bf16<W>(gfr, a.e.d0 + 2 * a.e.d1, a.e.d2, cur);
    }
    int off = 0, kin = a.e.K;
#pragma unroll 1
    for (int l = 0; l < a.e.n_layers; ++l) {
      off = chain_layer_fw<W>(s_mem, off, kin, a.e.layer[l].width, a.e.layer[l].op, cur);
      kin = a.e.layer[l].width;
    }
    if (live) {
      float* __restrict__ so = s_row + el * se;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < oe) so[k] = cur[k];
    }
  }
  // the slice is read by other lanes of this wave than wrote it: LDS operations of one wave execute in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- ef': the tile's run, each element rounded once ----
  chain_wave_store_run(s_row, a.inv_oe, a.ef_out, (r * (size_t)a.e.E + t.e0) * (size_t)oe, ne * oe, lane);

  // ---- the partial row's edge half: own rows in edge order, one tree per column ----
  float* __restrict__ prow = a.partials ? a.partials + (r * (size_t)a.n_wtiles + wt) * (size_t)(oe + on) : nullptr;
  if (prow) {
    float pe[W];
#pragma unroll
    for (int k = 0; k < W; ++k) pe[k] = 0.f;
    for (int base = 0; base < ne; base += 64) {
      const int el = base + lane;
      if (el < ne) {
        const float* __restrict__ so = s_row + el * se;
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < oe) pe[k] += so[k];
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < oe) { const float tot = wave_sum(pe[k]); mine = lane == k ? tot : mine; }
    if (lane < oe) prow[lane] = mine;
  }

  // ---- lanes as nodes ----
  const bool live = lane < nn;
  const int node = t.n0 + lane;
  float cur[W];
#pragma unroll
  for (int k = 0; k < W; ++k) cur[k] = 0.f;
  if (live) {
    const int c1 = a.n.colptr[node + 1] - t.e0;
    for (int i = a.n.colptr[node] - t.e0; i < c1; ++i) {
      const float* __restrict__ so = s_row + i * se;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < oe) cur[k] += so[k];
    }
    if (a.n.d1 > 0) chain_load_seg_bf16<W>(nf + (r * (size_t)a.n.N + node) * a.n.d1, oe, a.n.d1, cur);
    if (a.n.d2 > 0) chain_load_seg_bf16<W>(gfr, oe + a.n.d1, a.n.d2, cur);
  }
  int off = a.par_e, kin = a.n.K;
#pragma unroll 1
  for (int l = 0; l < a.n.n_layers; ++l) {
    off = chain_layer_fw<W>(s_mem, off, kin, a.n.layer[l].width, a.n.layer[l].op, cur);
    kin = a.n.layer[l].width;
  }
  if (prow) {
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < on) { const float tot = wave_sum(live ? cur[k] : 0.f); mine = lane == k ? tot : mine; }
    if (lane < on) prow[oe + lane] = mine;
  }

  // ---- nf': the rows over the slice (every lane is past its reads of ef'), then the tile's run ----
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (live) {
    float* __restrict__ so = s_row + lane * sn;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < on) so[k] = cur[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  chain_wave_store_run(s_row, a.inv_on, a.nf_out, (r * (size_t)a.n.N + t.n0) * (size_t)on, nn * on, lane);
}

struct ChainGraphWaveBf16Args {
  ChainMlpArgs f;          // the graph function: layers and K = oe + on + dg
  const float* partials;   // [R][n_wtiles][C]
  const bf16_t* gf;        // [R][G][dg]
  bf16_t* gf_out;          // [R][G][og]
  const int* wtile_off;    // [G + 1]
  int n_wtiles, C, dg, og, G, par;  // par: floats of the staged parameters
};

template <int W>
__global__ __launch_bounds__(1024) void k_chain_graph_wave_bf16(ChainGraphWaveBf16Args a) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int T = blockDim.x, tid = threadIdx.x, C = a.C;
  float* __restrict__ s_red = s_mem + a.par;  // [T] per-thread sums, then [C + dg] the function's input row
  float* __restrict__ s_x = s_red + T;
  chain_stage_params(a.f, s_mem, T);
  const int g = blockIdx.x;
  const size_t r = blockIdx.y;
  const int S = (T / C) * C;  // threads that add: thread t keeps column t % C
  const size_t n = (size_t)(a.wtile_off[g + 1] - a.wtile_off[g]) * C;
  const float* __restrict__ p = a.partials + (r * (size_t)a.n_wtiles + a.wtile_off[g]) * (size_t)C;
  float acc = 0.f;
  if (tid < S) {
    size_t i = tid;
    for (; i + 3 * (size_t)S < n; i += 4 * (size_t)S) {  // four loads in flight, added in element order
      const float x0 = p[i], x1 = p[i + S], x2 = p[i + 2 * (size_t)S], x3 = p[i + 3 * (size_t)S];
      acc += x0; acc += x1; acc += x2; acc += x3;
    }
    for (; i < n; i += S) acc += p[i];
  }
  s_red[tid] = acc;
  __syncthreads();
  if (tid < C) {
    float s = 0.f;
    for (int q = tid; q < S; q += C) s += s_red[q];
    s_x[tid] = s;
  } else if (tid < C + a.dg) {
    s_x[tid] = bf16_lo(a.gf[(r * (size_t)a.G + g) * a.dg + (tid - C)]);
  }
  __syncthreads();
  if (tid >= 64) return;
  float cur[W];
#pragma unroll
  for (int k = 0; k < W; ++k) cur[k] = k < a.f.K ? s_x[k] : 0.f;
  int off = 0, kin = a.f.K;
#pragma unroll 1
  for (int l = 0; l < a.f.n_layers; ++l) {
    off = chain_layer_fw<W>(s_mem, off, kin, a.f.layer[l].width, a.f.layer[l].op, cur);
    kin = a.f.layer[l].width;
  }
  if (tid == 0) {
    bf16_t* __restrict__ o = a.gf_out + (r * (size_t)a.G + g) * (size_t)a.og;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < a.og) o[k] = to_bf16(cur[k]);
  }
}

// launch_chain_wave on bf16 features and outputs.  The caller asked chain_wave_typed_takes; `partials`: R n_wtiles (oe + on) floats, the call's
// whole workspace.  The profiler names are the fp32 form's.
int32_t launch_chain_wave_bf16(const gnx_graphs* h, const gnx_chain_block_params& p, const ChainShape& sh, const void* ef, const void* nf, const void* gf, void* ef_out,
                               void* nf_out, void* gf_out, float* partials, int64_t R, hipStream_t s) {
  const int oe = sh.ow[0], on = sh.ow[1], og = sh.ow[2];
  auto cf = [](const void* q) { return static_cast<const float*>(q); };
  ChainWaveBf16Args a{};
  int we, wn;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, 0, p.edgefn, cf(ef), p.de, cf(nf), p.dn, cf(gf), p.dg, CHAIN_RULE_FW, "launch_chain_wave_bf16", s, a.e, &we, &rows)) return rc;
  if (int32_t rc = chain_mlp_prologue(h, 1, p.nodefn, nullptr, oe, cf(nf), p.dn, cf(gf), p.dg, CHAIN_RULE_FW, "launch_chain_wave_bf16", s, a.n, &wn, &rows)) return rc;
  a.waves = chain_wave_typed_waves(sh, h->wtile_e_cap);
  if (a.waves < 2 || h->max_in_degree > h->wtile_e_cap) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wave_bf16: the block is outside the wave rule");
  a.wtiles = h->d_wtiles; a.n_wtiles = (int)h->n_wtiles();
  a.slice = (int)chain_wave_typed_slice(sh, h->wtile_e_cap);
  a.par_e = (int)chain_narrow_lds_floats(p.edgefn, sh.k0[0]);
  a.par_all = a.par_e + (int)chain_narrow_lds_floats(p.nodefn, sh.k0[1]);
  a.ef_out = static_cast<bf16_t*>(ef_out); a.nf_out = static_cast<bf16_t*>(nf_out); a.partials = og > 0 ? partials : nullptr;
  a.oe = oe; a.on = on; a.inv_oe = chain_wave_inv(oe); a.inv_on = chain_wave_inv(on);
  {
    const dim3 grid((unsigned)((a.n_wtiles + a.waves - 1) / a.waves), (unsigned)R);
    const size_t lds = sizeof(float) * ((size_t)a.par_all + (size_t)a.waves * a.slice);
    ProfScope ps("k_rows_gemm_chain_e", s);
    const int w = std::max(we, wn);
    if (w <= 8) GNX_LAUNCH((k_chain_wave_bf16<8>), grid, dim3(64 * a.waves), lds, s, a);
    else if (w <= 16) GNX_LAUNCH((k_chain_wave_bf16<16>), grid, dim3(64 * a.waves), lds, s, a);
    else GNX_LAUNCH((k_chain_wave_bf16<32>), grid, dim3(64 * a.waves), lds, s, a);
    GNX_HIP(hipGetLastError());
  }
  if (og <= 0) return GNX_OK;
  ChainGraphWaveBf16Args b{};
  int wg;
  if (int32_t rc = chain_mlp_prologue(h, 2, p.graphfn, partials, sh.k0[2], nullptr, 0, nullptr, 0, CHAIN_RULE_FW, "launch_chain_wave_bf16", s, b.f, &wg, &rows)) return rc;
  b.partials = partials; b.gf = static_cast<const bf16_t*>(gf); b.gf_out = static_cast<bf16_t*>(gf_out); b.wtile_off = h->d_wtile_off;
  b.n_wtiles = a.n_wtiles; b.C = oe + on; b.dg = p.dg; b.og = og; b.G = (int)h->G;
  b.par = (int)chain_narrow_lds_floats(p.graphfn, sh.k0[2]);
  const int threads = graph_update_threads_for_rows(h->max_wtiles_per_graph);
  const size_t lds = sizeof(float) * ((size_t)b.par + threads + 64);
  ProfScope ps("k_rows_gemm_chain_g", s);
  const dim3 grid((unsigned)h->G, (unsigned)R);
  if (wg <= 8) GNX_LAUNCH((k_chain_graph_wave_bf16<8>), grid, dim3(threads), lds, s, b);
  else if (wg <= 16) GNX_LAUNCH((k_chain_graph_wave_bf16<16>), grid, dim3(threads), lds, s, b);
  else GNX_LAUNCH((k_chain_graph_wave_bf16<32>), grid, dim3(threads), lds, s, b);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
