/*
 * gnx.h — C ABI of libgnx.so: MI355X (gfx950) native GNBlock / GNCore forward for GraphNets.jl.
 *
 * The reference has no FFI; its boundary for this path is the Julia callable API exported at
 * src/GraphNets.jl:12-50.  Each entry point below names the reference interface it replaces; the Julia-side
 * `ccall` binding a maintainer would add is shown in INTEGRATION.md (and shipped in julia/GraphNetsHIP.jl).
 *
 * Conventions
 *   - Every function returns int32 status: 0 = GNX_OK; < 0 = invalid argument (mirrors an `@assert` of the
 *     reference, src/checks.jl, src/batch.jl:54-56, src/gnblock.jl:48-49); > 0 = a hipError_t value.  A
 *     message is available from gnx_last_error() (thread-local).  Nothing throws across the ABI.
 *   - Feature buffers are DEVICE pointers, fp32, packed rows: ef [R][E][DE], nf [R][N][DN], gf [R][G][DG]
 *     (row-major) — byte-identical to Julia's column-major (D, T, R) arrays and, for vector-of-graphs
 *     batches (R = 1), to flatunpaddedef / flatunpaddednf (src/views.jl:80-98).  R = number of replicas of
 *     the graph structure: the data batch size B of a shared-adjacency batch (src/batch.jl:66), 1 otherwise.
 *     E, N, G are totals over the graphs of the handle.  NULL <=> `nothing`; the (DE, 0) edge features of a batch WITHOUT
 *     edges have no bytes and may be NULL too (their width still counts: sums over them are rows of DE zeros).
 *   - Edge order inside a graph = order of the ones of vec(A) column-major (src/pad.jl:30): sorted by
 *     destination j then source i, A[i,j] = 1 meaning i -> j (src/gngraphbatch.jl:194-211).
 *   - Dense weights are (out x in) column-major = Flux `Dense.weight` bytes: W[k*out + j]; device pointers.
 *   - The caller owns every buffer; the library owns only gnx_graphs handles (and, for gnx_model, the model's intermediate
 *     tensors).  `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on it and hipGraph-capturable (no
 *     allocation, no sync) with four documented exceptions that happen once, outside any capture: the first use of a width
 *     set that needs a run-time specialised kernel (see gnx_jit_*), the first backward / edge-collapsing call on a handle
 *     (builds the CSR / collapse tables of the handle), the handle's matrix-core tables (widths from 32: built by the
 *     gnx_*_workspace_bytes query of the layer — every caller runs that query before a forward, outside a capture; a forward,
 *     backward or gnx_fn_input(kind 0) that still finds them missing builds them itself, or, when its stream is being captured,
 *     fails with GNX_ERR_INVALID_ARG and a message saying so — not remembered: the next call outside the capture succeeds), and
 *     gnx_model_forward (which manages its own hipGraph).
 *   - The library uses the calling thread's current HIP device; a handle lives on the device it was created on.
 *   - Output buffers must not overlap input buffers or the workspace (the kernels read inputs while they write outputs; the training forward
 *     re-reads x after the outputs exist).  The reference's layers are out-of-place as well (every update allocates its result).
 *   - Sizes are exact: a feature / gradient buffer is R * T * D * sizeof(element) bytes, a workspace the value of its gnx_*_workspace_bytes
 *     query; a call writes nothing outside its output, gradient and workspace buffers, leaves its inputs (features, weights, upstream
 *     gradients) untouched, and its result does not depend on what the workspace held before — except between the phases of the forms that
 *     say so (GNX_FLAG_DEFER_GRAPH_UPDATE -> gnx_block_graph_update, gnx_block_forward_chained, the steps of gnx_block_forward_steps).
 *     tests/test_gpu_memory_contract.py holds every dispatch form to this.
 *   - Alignment: every public entry point accepts fp32 and bf16 buffers (features, weights, biases, LayerNorm gamma / beta, upstream and
 *     input gradients, parameter gradients) that are 4-byte aligned (a bf16 buffer too: GNX_ERR_INVALID_ARG below that; its rows of odd width
 *     are then 2-byte aligned); only the workspace needs 16 bytes (GNX_ERR_WORKSPACE otherwise, before anything is written).  The narrow and
 *     generic kernels assume no more than the 4 bytes.  The matrix-core launchers (any width above 32: csrc/gnx_wide.hip, gnx_edge_x6.hip,
 *     gnx_ffn_*.hip, gnx_backward_wide.hip) TEST 16-byte alignment of the pointers they are handed — and of the replica strides R > 1 adds to
 *     them — and take an element-wise or another kernel form when it does not hold; the six-term kernels need their bias and LayerNorm gamma /
 *     beta vectors 16-byte aligned, and the plans (wide_plan, the core's form decision) take another form when they are not: a launcher's own
 *     refusal of such a vector is an internal defence no public call reaches.  Results at another alignment meet the same bounds; where no
 *     summation order depends on an address (narrow, generic and bf16 kernels) they are the same bits.  Tested: tests/test_gpu_alignment.py
 *     runs every case of the memory-contract table with its buffers at 256 k + 4, + 8 and + 12 bytes — all of them at once, features only,
 *     parameters only, and one operand group at a time —, replica strides that are no multiple of 16 bytes, and the Python mirror on views
 *     into the middle of a tensor; tests/test_arena_cpu.py counts the pointer-alignment tests of csrc/ so that a new one comes with its case.
 */
#ifndef GNX_H
#define GNX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNX_VERSION 130 /* 0.1.3: gnx_block_forward_steps; no default path on the fp32 matrix instruction; 120: training-mode Dropout (gnx_dropout, gnx_core_forward_train / _backward_train); 110: gnx_profile_entry is 72 bytes, per-call arithmetic flags, prepared parameters, GNX_FLAG_DIST_NO_GATHER */

#if defined(__GNUC__)
#define GNX_API __attribute__((visibility("default")))
#else
#define GNX_API
#endif

/* status codes (negative = argument errors, named after the reference assertion they mirror) */
#define GNX_OK 0
#define GNX_ERR_INVALID_ARG (-1)   /* NULL where a pointer is required, negative size, bad enum            */
#define GNX_ERR_NO_GRAPHS (-2)     /* checks.jl:8    @assert length(adj_mats) > 0                           */
#define GNX_ERR_ADJ_SHAPE (-3)     /* checks.jl:11   adjacency must be square (N x N), N >= 1               */
#define GNX_ERR_ADJ_VALUE (-4)     /* gngraphbatch.jl:207 / pad.jl:30  entries must be 0 or 1               */
#define GNX_ERR_ALL_NOTHING (-5)   /* batch.jl:56    ef, nf, gf all `nothing`                               */
#define GNX_ERR_DIMS (-6)          /* gnblock.jl:48-49, gnfeedforward.jl:18, gngraphnorm.jl:10              */
#define GNX_ERR_CSC (-7)           /* malformed CSC: colptr not monotone, rowval out of range / unsorted    */
#define GNX_ERR_WORKSPACE (-8)     /* workspace NULL or smaller than gnx_*_workspace_bytes()                */
#define GNX_ERR_TOO_LARGE (-9)     /* N or E does not fit the int32 device indices                          */
#define GNX_ERR_COUNT_MISMATCH (-10) /* checks.jl:41-46 size(ef,2)==num_edges, size(nf,2)==num_nodes — raised by the host
                                      * shims (the ABI sees pointers only); reserved here so the codes stay in one place  */

/* activations (Flux/NNlib): identity is the GNBlock default (gnblock.jl:55-60); relu is used by FeedForward */
#define GNX_ACT_IDENTITY 0
#define GNX_ACT_RELU 1
#define GNX_ACT_TANH 2
#define GNX_ACT_SIGMOID 3
#define GNX_ACT_GELU 4 /* NNlib.gelu (tanh form) */

/* element kinds of dense adjacency input */
#define GNX_ELEM_U8 0
#define GNX_ELEM_I32 1
#define GNX_ELEM_I64 2
#define GNX_ELEM_F32 3
#define GNX_ELEM_F64 4
/* bfloat16: FEATURE tensors only (gnx_block_forward_typed); the adjacency constructors reject it like any other unknown kind */
#define GNX_ELEM_BF16 5

/* forward flags */
#define GNX_FLAG_FORCE_GENERIC 0x1u /* use the dimension-generic kernels even when a specialised path exists */
#define GNX_FLAG_NO_MFMA 0x2u       /* never pick the MFMA path                                               */
#define GNX_FLAG_DEFER_GRAPH_UPDATE 0x4u /* gnx_block_forward stops after the edge+node update and leaves the per-tile
                                          * partial sums in the workspace; gnx_block_graph_update finishes gf' later   */

/* FORMS of the forward, selected PER CALL (every gnx_*_forward / gnx_model_forward / gnx_dist_* takes them in `flags`; the reference's layers
 * are stateless values, src/gnblock.jl:63-69 — which arithmetic a call runs is an argument of the call, not a property of the process).
 * Each has an environment variable of the same name (GNX_FFN_FP32=1 ...) that is read ONCE per process, at the first library call, and OR-ed
 * into every call's flags as the process-wide default (gnx_default_flags() returns that mask); the library never calls getenv() on a forward. */
#define GNX_FLAG_FFN_FP32 0x20u   /* wide GNCore FeedForwards on the fp32 matrix instruction (k_ffn_fused) instead of six bf16 terms (k_ffn_x6) */
#define GNX_FLAG_EDGE_FP32 0x40u  /* projected edge update and node projections on the fp32 matrix instruction (k_rows_gemm) instead of six bf16 terms */
#define GNX_FLAG_FP32_MFMA (GNX_FLAG_FFN_FP32 | GNX_FLAG_EDGE_FP32) /* every matrix product of the call on the fp32 matrix instruction */
#define GNX_FLAG_PROJ_FP32 0x80u          /* the node-side kernels alone (node projections, node update) on the fp32 instruction            */
#define GNX_FLAG_EDGE_NARROW_FP32 0x100u  /* the 128 -> (<= 32) edge update alone on the fp32 instruction                                  */
/* diagnostic forms — same results (bit-identical where the header says so), kept for A/B runs and for the tests that compare two forms */
#define GNX_FLAG_NO_LN_FUSE 0x200u       /* wide GNCore: materialise gn1 / gn2 (k_layernorm2) instead of normalising on load               */
#define GNX_FLAG_LN_STATS_PASS 0x400u    /* wide GNCore: row statistics of ef by the statistics pass instead of in the six-term kernels    */
#define GNX_FLAG_CORE_EDGE_SPLIT 0x800u  /* wide GNCore: edge update and edge FeedForward as two launches                                  */
#define GNX_FLAG_NO_FORK 0x1000u         /* wide GNCore: everything on the caller's stream (no side stream for the graph level)            */
                                         /* ... and gnx_block_forward_steps: every step on the caller's stream (no two-stream schedule)    */
#define GNX_FLAG_NO_PACK 0x2000u         /* narrow block on small graphs: graph update as its own launch (k_graph_t)                       */
#define GNX_FLAG_NO_FFE 0x4000u          /* narrow GNCore: edge FeedForward in k_core_post3 instead of the block kernel's edge lanes       */
#define GNX_FLAG_NO_JIT 0x8000u          /* never specialise a kernel at run time (generic kernels instead); env GNX_JIT=0 / GNX_NO_JIT=1   */
#define GNX_FLAG_EDGE_N 0x10000u         /* opt-in: k_edge_n (source rows gathered raw, K = 128 + 64; csrc/gnx_edge_n.hip) for the edge update */
#define GNX_FLAG_LN_ON_LOAD 0x20000u     /* wide GNCore: normalise on load from a row-statistics table also where a GENERAL kernel (k_rows_gemm, k_ffn_fused)
                                          * consumes it — rounds 2-5's default; round 6 materialises those LayerNorms instead (csrc/gnx_forward.hip,
                                          * profiles/r06_overlap_hazard.log); the same formula, exact too since that branch is guarded      */
#define GNX_FLAG_FORMS_MASK 0x3ffe0u
GNX_API uint32_t gnx_default_flags(void); /* the forms the environment switched on for this process */

typedef struct gnx_graphs gnx_graphs; /* opaque; replaces GNGraphBatch (src/gngraphbatch.jl:1-54) */

typedef struct gnx_graphs_info {
  int64_t n_graphs;        /* G = length(adj_mats)                                   */
  int64_t n_nodes;         /* sum of N_g                                             */
  int64_t n_edges;         /* sum of E_g                                             */
  int64_t node_block_size; /* PN = max N_g           (gngraphbatch.jl:35)            */
  int64_t edge_block_size; /* PN^2                   (gngraphbatch.jl:36)            */
  int64_t n_tiles;         /* work tiles (node ranges) the kernels iterate over      */
  int64_t max_in_degree;
  int32_t device;
  int32_t reserved;
} gnx_graphs_info;

/* One Flux `Dense(in => out, act)`: y = act.(W*x .+ b).  bias may be NULL (= zeros).
 * `kind` (0 everywhere but inside a gnx_chain): GNX_LAYER_LAYERNORM makes the entry a Flux `LayerNorm(d)` layer value of a Chain — weight =
 * gamma [d], bias = beta [d], act = identity, its width = the width of its input, eps = 1e-5 (Flux's default), (x - mean) / (sigma + eps)
 * (Flux 0.14 `normalise`; `| GNX_LAYER_LN_SQRT_EPS`: / sqrt(sigma^2 + eps)).  gnx_block_params' three functions must be Dense (kind 0). */
#define GNX_LAYER_DENSE 0
#define GNX_LAYER_LAYERNORM 1
#define GNX_LAYER_LN_SQRT_EPS 0x100
typedef struct gnx_dense {
  const float* weight; /* (out x in) column-major, device; LayerNorm entry: gamma [d] */
  const float* bias;   /* (out), device, or NULL;          LayerNorm entry: beta [d]  */
  int32_t act;         /* GNX_ACT_*                       */
  int32_t kind;        /* GNX_LAYER_* (was `reserved`: 0 = Dense) */
} gnx_dense;

/* Prepared parameters (opaque): a layer's weight blocks in the forms the matrix-core kernels stage (bf16 planes of the exact three-way
 * split, transposed, slot-permuted) — made ONCE per upload of the weights by gnx_block_prepare / gnx_core_prepare below instead of by
 * preparation launches in front of every forward (`model |> device` happens once: examples/sort/sort.jl:29,89). */
typedef struct gnx_prepared gnx_prepared;

/* GNBlock((de,dn,dg) => (oe,on,og)) (src/gnblock.jl:47-61): edgefn in = de+2dn+dg, nodefn in = oe+dn+dg
 * (order agg, nf, gf: nodefninput.jl:2-6), graphfn in = oe+on+dg (order edges, nodes, gf: graphfninput.jl:2-6). */
typedef struct gnx_block_params {
  int32_t de, dn, dg; /* input widths; 0 <=> that input is `nothing` */
  int32_t oe, on, og; /* output widths; 0 <=> that output is `nothing` (gnblock.jl:71-78) */
  gnx_dense edgefn, nodefn, graphfn;
  const gnx_prepared* prepared; /* gnx_block_prepare's result for THESE weights, or NULL (the forward then prepares them per call) */
} gnx_block_params;

typedef struct gnx_layernorm { /* Flux LayerNorm(d): gamma .* xhat .+ beta */
  const float* gamma;
  const float* beta;
} gnx_layernorm;

typedef struct gnx_ffn { /* FeedForward (gnfeedforward.jl:27-31): Dense(d=>4d, relu), Dense(4d=>d); Dropout = identity */
  gnx_dense fc1, fc2;
} gnx_ffn;

/* GNCore(dims) (src/gncore.jl:46-59): y = x + block(gn1(x)) + ffwd(gn2(x)); index 0/1/2 = edge/node/graph. */
typedef struct gnx_core_params {
  gnx_block_params block; /* dims => dims */
  gnx_layernorm ln1[3], ln2[3];
  gnx_ffn ff[3];
  float eps;        /* 1e-5 */
  int32_t eps_mode; /* 0: (x-mu)/(sigma+eps) (Flux 0.14 normalise);  1: (x-mu)/sqrt(sigma^2+eps) */
  const gnx_prepared* prepared; /* gnx_core_prepare's result for THESE weights (block and FeedForwards), or NULL; block.prepared is ignored */
} gnx_core_params;

typedef struct gnx_profile_entry {
  char name[48];
  int64_t launches; /* times the named scope was entered (one per step for most scopes)                  */
  double total_ms;  /* sum of the dispatch-timestamp durations of every kernel launched inside the scope */
  int64_t kernels;  /* kernels launched inside the scope (the graph level of a wide block: three per entry) */
} gnx_profile_entry;

/* ---- library ---- */
GNX_API int32_t gnx_version(void);
GNX_API const char* gnx_last_error(void);

/* ---- graph handles: replace batchgraphs / GNGraphBatch(adj_mats) (src/batch.jl:66-67, src/gngraphbatch.jl:33-54) ---- */

/* adj[g] points at an n_nodes[g] x n_nodes[g] matrix of `elem_kind`, HOST memory; `row_major` = 0 for Julia
 * (column-major) input, 1 for C/numpy.  Entries must be exactly 0 or 1. */
GNX_API int32_t gnx_graphs_create_dense(const void* const* adj, const int64_t* n_nodes, int64_t n_graphs, int32_t elem_kind,
                                int32_t row_major, gnx_graphs** out);

/* The same batch from ONE buffer: the matrices one after the other (graph g: n_g x n_g elements of elem_kind), adj_bytes = sum(n_g^2) *
 * sizeof(element) — checked; nothing is read past it.  on_device = 0: HOST memory (a pinned buffer travels as one DMA, a pageable one through
 * the library's pinned staging pair); on_device = 1: DEVICE memory of the current device (no copy; the scan runs on the NULL
 * stream: the buffer must be COMPLETE when the call is made — a producer on a non-blocking stream is synchronised by the caller first, as the
 * Python mirror does).  What a data loader holds and what the
 * bindings call (GNGraphBatch.from_dense_packed): one pointer instead of G — building G pointers costs a Python / Julia host ~1.5 us each. */
GNX_API int32_t gnx_graphs_create_dense_packed(const void* adj_cat, int64_t adj_bytes, const int64_t* n_nodes, int64_t n_graphs, int32_t elem_kind,
                                       int32_t row_major, int32_t on_device, gnx_graphs** out);

/* Per-graph CSC (Julia SparseMatrixCSC colptr / rowval, HOST memory): colptr[g] has n_nodes[g]+1 entries,
 * rowval[g] the local source index of every edge, sorted strictly increasing inside a column; index_base is 1
 * for Julia arrays, 0 for C.  The nz order of CSC *is* the reference edge order.  (API extension: the reference
 * only accepts dense matrices, which cannot hold BASELINE configs 2-5.) */
GNX_API int32_t gnx_graphs_create_csc(const int64_t* const* colptr, const int64_t* const* rowval, const int64_t* n_nodes,
                              int64_t n_graphs, int32_t index_base, gnx_graphs** out);
/* the same batch from TWO arrays: colptr_cat = the graphs' colptr arrays one after the other (n_g + 1 entries each, every one starting at
 * index_base), rowval_cat = their rowval arrays one after the other.  One call and two pointers instead of 2 G pointers: what a host
 * pays per graph to build pointer arrays (8 ms for 4096 graphs through ctypes) is the larger part of batch() on many small graphs. */
GNX_API int32_t gnx_graphs_create_csc_packed(const int64_t* colptr_cat, const int64_t* rowval_cat, const int64_t* n_nodes, int64_t n_graphs,
                                     int32_t index_base, gnx_graphs** out);

/* the packed form WITH its array lengths and index width — what a host binding should call: colptr_cat / rowval_cat hold colptr_len /
 * rowval_len indices of index_bits (32 or 64) bits each; the call fails with GNX_ERR_INVALID_ARG unless colptr_len = sum(n_nodes) + n_graphs
 * and rowval_len = the edges the colptr arrays announce, and never reads past either length whatever the arrays contain. */
GNX_API int32_t gnx_graphs_create_csc_cat(const void* colptr_cat, int64_t colptr_len, const void* rowval_cat, int64_t rowval_len,
                                  const int64_t* n_nodes, int64_t n_graphs, int32_t index_base, int32_t index_bits, gnx_graphs** out);

GNX_API int32_t gnx_graphs_destroy(gnx_graphs* h);
GNX_API int32_t gnx_graphs_get_info(const gnx_graphs* h, gnx_graphs_info* out);
/* host copies, 0-based: node_off[G+1], edge_off[G+1] (what unpadnf/unpadef/efview/nfview index with,
 * src/unpad.jl:1-25, src/views.jl:6-98); any pointer may be NULL */
GNX_API int32_t gnx_graphs_get_offsets(const gnx_graphs* h, int64_t* node_off, int64_t* edge_off);
/* host copies, 0-based global CSC: colptr[N+1], rowval[E] (global source node id) */
GNX_API int32_t gnx_graphs_get_csc(const gnx_graphs* h, int64_t* colptr, int64_t* rowval);

/* diagnostic: one of the handle's DEVICE tables copied to the host as it is — which = 0 colptr [N+1] int32, 1 rowval [E] int32 (global source
 * ids), 2 node_off, 3 edge_off, 4 tile_off [G+1] int32, 5 workgroup tiles (32-byte records {n0, n1, e0, e1, g, win0, win1, flags}), 6 wtile_off,
 * 7 wave tiles, 8 packs [n_packs][8] int32; 9..18 the matrix-core path's tables (built on the spot if they are not yet: 9 edge tiles, 10 node
 * tiles, 11 graph tiles, 12 / 13 their per-graph offsets, 14 destination of every edge, 15 first partial-sum row of every aggregation chunk,
 * 16 / 17 / 18 per node: its partial-sum row, the chunks its in-edges run through, its first chunk), 19 five int64 {partial-sum rows, edge tiles
 * with a wide destination span, edge / node / graph tile counts}.  *bytes = the table's size (out may be NULL to ask for it).  Large batches given as CSC are
 * validated and tiled by kernels (env GNX_BUILD_CSC_DEVICE=0: on the host); the two builders' tables are bit-identical (tests/test_gpu_build.py). */
GNX_API int32_t gnx_graphs_get_table(const gnx_graphs* h, int32_t which, void* out, int64_t capacity_bytes, int64_t* bytes);

/* ---- prepared parameters ----
 * gnx_block_prepare / gnx_core_prepare read the DEVICE weights the descriptor points at (on `stream`, asynchronously) and return an object
 * to put into the descriptor's `prepared` field.  A forward whose descriptor carries it launches no preparation kernel (config 4: nine
 * launches, ~45 us, per forward otherwise); outputs are bit-identical either way.  The planes are looked up by the weight POINTERS the
 * forward is handed: a prepared object made from other weights, or on another device, is simply not used.  Contract: the parameters' VALUES
 * must not change while a prepared object made from them is in use — after an optimiser step call gnx_prepared_refresh (same stream
 * order as the update), and destroy the object before the parameters are freed.  "Parameters" is the weights and, for a core with 128-wide
 * edges, gn1 / gn2's gamma and beta of the edges and the edge FeedForward's first bias: the one-launch form of the core's edge rows has
 * them folded into its planes ((gamma . W)^T xhat + W^T beta; the rows are normalised and split once).  Widths without a six-term kernel prepare nothing (an empty
 * object).  gnx_model_create prepares the layers whose descriptors carry none (see gnx_model_refresh_weights). */
GNX_API int32_t gnx_block_prepare(const gnx_block_params* p, void* stream, gnx_prepared** out);
GNX_API int32_t gnx_core_prepare(const gnx_core_params* p, void* stream, gnx_prepared** out);
GNX_API int32_t gnx_prepared_refresh(gnx_prepared* q, void* stream);
GNX_API int32_t gnx_prepared_destroy(gnx_prepared* q);
GNX_API int64_t gnx_prepared_bytes(const gnx_prepared* q); /* device memory the object holds */

/* ---- forward: replaces (m::GNBlock)(x) (src/gnblock.jl:63-69) ---- */
GNX_API size_t gnx_block_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_block_forward(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf,
                          const float* gf, int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out,
                          void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* The same forward on bfloat16 feature tensors.  `elem` (GNX_ELEM_F32 or GNX_ELEM_BF16) applies to all six tensors; GNX_ELEM_F32 is exactly
 * gnx_block_forward.  Contract, for finite data: the bf16 result is bit for bit to_bf16(gnx_block_forward(widen(ef), widen(nf), widen(gf)))
 * under the same flags — inputs are widened exactly, every intermediate (edge->node sums, graph-update partial sums, workspace) stays fp32,
 * and only the three outputs are rounded, to nearest even.  bf16 buffers must be 4-byte aligned (rows of odd width are then 2-byte aligned:
 * the kernels never assume more).  Paths: the fused narrow kernel reads and writes bf16 rows itself (ahead of time for README ex.1's widths,
 * run-time specialised for every other narrow width set); every other path — matrix-core / generic widths, GNX_FLAG_FORCE_GENERIC,
 * GNX_FLAG_NO_JIT, a failed specialisation — widens the inputs into fp32 staging buffers of the workspace, runs gnx_block_forward on them
 * and rounds the outputs.  gnx_block_typed_workspace_bytes sizes the workspace for the path these flags take (the staging only when it is
 * needed; the process-wide default forms are ORed in as everywhere) and compiles / loads a run-time specialisation, so call it outside any
 * capture; it returns 0 for an unknown `elem` or GNX_FLAG_DEFER_GRAPH_UPDATE with bf16, which gnx_block_forward_typed rejects
 * (GNX_ERR_INVALID_ARG) before any GPU work.  No allocation, no synchronisation: capture-safe like gnx_block_forward. */
GNX_API size_t gnx_block_typed_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem, uint32_t flags);
GNX_API int32_t gnx_block_forward_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const void* ef, const void* nf, const void* gf,
                                        int64_t n_replicas, void* ef_out, void* nf_out, void* gf_out, void* workspace, size_t workspace_bytes,
                                        uint32_t flags, void* stream);

/* Second phase of a deferred block forward: gf'[g] = graphfn([sum_e ef' ; sum_n nf' ; gf_g]) (src/gnblock.jl:67,
 * src/graphfninput.jl:1-13) from the partial sums a gnx_block_forward(..., GNX_FLAG_DEFER_GRAPH_UPDATE, ...) call left
 * in `workspace` (same handle, params, n_replicas, flags and workspace; the workspace must not be reused in between).
 * It is a few KB of work that only the caller of gf' waits for: launched on a second stream (after an event recorded
 * behind the first phase) it overlaps the next batch's edge/node update instead of sitting on the critical path. */
GNX_API int32_t gnx_block_graph_update(const gnx_graphs* h, const gnx_block_params* p, const float* gf, int64_t n_replicas,
                               float* gf_out, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* ---- the graph update of call i inside call i + 1: loops over many batches of the same graphs (serving, training) -------------------------
 * A block forward at README widths is one ~19-us kernel plus a second launch that finishes gf' from a few KB of partial sums (~4 us, what an
 * EMPTY launch costs, + the boundary).  gnx_block_forward_chained runs this call's edge + node update and — in workgroups at the FRONT of
 * the same launch — the graph update that the previous chained call left pending (`prev`: that call's workspace, gf and gf_out, as the
 * library recorded them; NULL or zeroed: nothing pending).  On return *pending describes THIS call's pending graph update: its gf_out is
 * valid only after the next chained call on this stream or after gnx_block_graph_update(h, p, pending->gf, R, pending->gf_out,
 * pending->workspace, pending->workspace_bytes, flags, stream) (the flush; pending->workspace == NULL: nothing to flush).  Same handle,
 * params, n_replicas and flags in consecutive calls; the pending call's workspace and gf_out must differ from this call's (two alternating
 * buffer sets).  Where the two-launch form is not what runs (matrix-core / generic kernels, run-time specialised widths, batches of small
 * graphs whose graph update already runs inside the block kernel) the call finishes `prev` and this call the plain way and leaves nothing
 * pending.  Results are bit-identical to gnx_block_forward's (the same graph_update_rows over the same partial rows). */
typedef struct gnx_pending_update {
  const void* workspace;
  size_t workspace_bytes;
  const float* gf;
  float* gf_out;
} gnx_pending_update;
GNX_API int32_t gnx_block_forward_chained(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf, const float* gf,
                                  int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out, void* workspace, size_t workspace_bytes,
                                  uint32_t flags, void* stream, const gnx_pending_update* prev, gnx_pending_update* pending);

/* ---- a LOOP over batches as ONE call (round 6): what `for x in batches; y = block(x); end` is in a serving / evaluation loop over resident
 * batches of the same graphs (examples/sort/sort.jl:99-108 walks its batches this way).  Exactly n_steps gnx_block_forward calls in order —
 * the same kernels over the same rows, outputs bit-identical — but the library KNOWS the next step exists, so where the two-launch narrow
 * form runs it uses the chained form above by itself: step i's graph update rides at the front of step i + 1's launch, the last step's is
 * flushed before the call returns its work to the stream (ONE launch per step + one flush instead of two launches per step: 22.2 vs 25.1
 * us/step on BASELINE configs[1]).  Every output of every step is complete once the work this call enqueued is complete.  Consecutive
 * steps must not share a workspace or a gf_out (step i + 1 starts while step i's graph update is pending): a step that does share them with
 * its predecessor is simply run unchained.  Other paths (matrix-core / generic kernels, batches of small graphs): n_steps plain forwards.
 * Capture-safe like gnx_block_forward (bench.py captures K steps into one hipGraph).
 * TWO STREAMS: where the fused narrow kernel runs (plain, chained, pack form, run-time specialised widths) even steps go to the caller's
 * stream and odd steps to a side stream of the handle's pool (gnx_block_workspace_bytes creates it, outside any capture), forked from and
 * joined back into `stream` inside the call (on error paths too), so neighbouring steps overlap; the chained graph update of step i then
 * rides at the front of step i + 2's launch (its stream's next), and two pending updates are flushed at the end.  Steps whose buffers
 * overlap (one step writes a byte range — ef_out, nf_out, gf_out, workspace — that another reads or writes, up to three steps apart) are
 * ordered by an event wait instead, and every step's launch waits for the end of the launch three steps before it (the streams never
 * drift further apart).  Outputs are bit-identical in either schedule.  One stream: GNX_FLAG_NO_FORK, matrix-core / generic
 * kernels, the per-kernel profiler on (gnx_profile_enable), or every side stream of the handle taken by other host threads.
 * RUNS: neighbouring steps whose buffers do not overlap may SHARE A LAUNCH.  Where the chained form would run and the width set has a
 * run kernel (the narrow ahead-of-time sets, fp32 and bf16, n_replicas == 1) the library groups consecutive steps, by the same
 * address-range rule, into runs of GNX_STEPS_RUN_MAX steps (environment, read once; default 8, at most 8; 1: every step its own launch):
 * a run is ONE block launch with a slot per step plus one launch for their graph updates, and "step" in the two-stream schedule above
 * reads "run".  Only a full run, or the last four or more steps of the loop, share a launch (shorter ones measured no gain): where a
 * conflict cuts the window short (a shared workspace or gf_out, dims -> dims feedback, fewer buffer sets in rotation than that)
 * the step is a run of its own — the chained step above.  Unchanged: the order of the results, their bits (each slot is
 * the program of a launch of its own), and that every output is complete, and the side stream joined, when the call returns its work to
 * `stream` — on error paths too; a step's argument error is reported once everything before it has been issued, and an invalid step
 * never joins a run.  With the per-kernel profiler on every run is one step (its figures are per step). */
typedef struct gnx_block_step {
  const float* ef;
  const float* nf;
  const float* gf;
  float* ef_out;
  float* nf_out;
  float* gf_out;
  void* workspace;
  size_t workspace_bytes; /* >= gnx_block_workspace_bytes */
} gnx_block_step;
GNX_API int32_t gnx_block_forward_steps(const gnx_graphs* h, const gnx_block_params* p, const gnx_block_step* steps, int64_t n_steps,
                                int64_t n_replicas, uint32_t flags, void* stream);

/* The same loop on bfloat16 feature tensors.  GNX_ELEM_F32 is exactly gnx_block_forward_steps.  With GNX_ELEM_BF16 the six feature pointers
 * of every step point to bf16 storage (they keep their float* type in gnx_block_step) and each step's workspace_bytes is at least
 * gnx_block_typed_workspace_bytes(h, p, n_replicas, GNX_ELEM_BF16, flags) — the query that also creates the side streams, outside any capture.
 * Contract, for finite data: each step's outputs are bit for bit those of gnx_block_forward_typed on that step alone, the steps run in order —
 * in every schedule (one stream, two streams, chained, replayed from a captured graph).  Where a native bf16 kernel takes the widths (the
 * ahead-of-time sets, run-time specialised widths, the pack form) the loop runs the schedule above on bf16 rows: two streams, and step i's
 * graph update at the front of a later launch at the bf16 ahead-of-time widths (the chained graph update reads the previous step's fp32
 * partial rows and its bf16 gf, and rounds its gf_out as k_graph_t does); one stream under GNX_FLAG_NO_FORK, the profiler or an exhausted
 * pool, still chained.  Every other path (matrix-core / generic widths, GNX_FLAG_FORCE_GENERIC, GNX_FLAG_NO_JIT, a failed specialisation):
 * n_steps gnx_block_forward_typed calls in order on `stream`, each converting around the fp32 forward inside its own workspace.
 * Refused with GNX_ERR_INVALID_ARG BEFORE ANY GPU WORK: an `elem` other than these two, GNX_FLAG_DEFER_GRAPH_UPDATE, a negative n_steps or
 * steps == NULL with n_steps > 0, and a feature buffer of ANY step that is not 4-byte aligned.  (Unlike gnx_block_forward_steps, which reports a
 * step's error once the steps before it have been issued.)  An error found only inside the loop (a workspace too small, a NULL input) is
 * reported once the steps before it are issued, with the side stream joined into `stream` as in the fp32 loop.  There is no typed
 * gnx_block_forward_chained or gnx_block_graph_update: the pending graph updates stay inside this call. */
GNX_API int32_t gnx_block_forward_steps_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const gnx_block_step* steps,
                                              int64_t n_steps, int64_t n_replicas, uint32_t flags, void* stream);

/* ---- GNBlock with Flux `Chain`s of Dense layers as update functions (src/gnblock.jl:1-6: edgefn / nodefn / graphfn are
 * arbitrary Chains; the constructor's default is Chain(Dense), which is what gnx_block_forward fuses).  widths[i] = output
 * width of layer i; the input width of layer 0 is fixed by the block (de+2dn+dg / oe+dn+dg / oe+on+dg with oe, on = the LAST
 * widths of the edge / node chains); a chain with n_layers = 0 or a last width of 0 <=> that output is `nothing`.
 * The edge function's first layer runs fused with getedgefninput (the fast block kernels); every further layer is a row-wise
 * Dense on the matrix-core GEMM kernel.  A layer entry may also be a `LayerNorm(d)` layer value (gnx_dense.kind = GNX_LAYER_LAYERNORM,
 * `Chain(Dense(a => d, relu), LayerNorm(d), Dense(d => b))`: normalised rows of the layer in front, its width = that layer's) — anywhere in a chain;
 * as the edge function's FIRST layer it runs behind an identity Dense that the library puts in front (the fused launch then writes the
 * function input itself: K_e x K_e floats more of workspace).  The gradient entries of a LayerNorm layer are (gamma, beta).
 * Backward: gnx_chain_block_backward below. */
typedef struct gnx_chain {
  const gnx_dense* layers; /* [n_layers] host array of layer descriptors (device weight pointers inside) */
  const int32_t* widths;   /* [n_layers] host array */
  int32_t n_layers;
  int32_t reserved;
} gnx_chain;
typedef struct gnx_chain_block_params {
  int32_t de, dn, dg; /* input widths; 0 <=> nothing */
  int32_t reserved;
  gnx_chain edgefn, nodefn, graphfn;
} gnx_chain_block_params;
GNX_API size_t gnx_chain_block_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_chain_block_forward(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf,
                                int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out, void* workspace, size_t workspace_bytes,
                                uint32_t flags, void* stream);
/* The same block with each update function in ONE kernel where its widths are narrow: a row of the entity lives in one lane's registers, is
 * built there (edge: [ef ; nf[src] ; nf[dst] ; gf_g], node: [sum of the incoming ef' in CSC order ; nf ; gf_g], graph: the materialised
 * getgraphfninput rows) and runs through ALL layers of the function — Dense with any activation, LayerNorm layer values, a LayerNorm as the
 * edge function's first layer without an identity Dense in front — with the function's parameters staged in LDS.  The rule is per update
 * function.  A function is fused when it has at least one layer and a non-zero output width, its input width and every layer width are at
 * most 32, its zero-padded parameters (a Dense: ceil4(k_in) * ceil4(width) + ceil4(width) floats, a LayerNorm: 2 * ceil4(width), ceil4 = rounded
 * up to a multiple of 4) fit the kernel's LDS budget of 10240 floats (40 KB), and its entity has rows.
 * _applies: bit 0 the edge, bit 1 the node, bit 2 the graph function is fused; 0 on bad arguments.  _workspace_bytes: a fused function has
 * none of the hidden-row / input buffers (the graph function keeps its G input rows); it builds the handle's tables the call reads, so call it
 * outside a stream capture.  A function outside the rule runs exactly gnx_chain_block_forward's launches for it; with a mask of 0 the call IS
 * gnx_chain_block_forward (same workspace size, same bits).  A fused function's results are plain fp32 FMA chains in layer order: within the
 * library's 1e-5 bound of gnx_chain_block_forward's, not its bits.  Arguments and refusals as gnx_chain_block_forward. */
GNX_API int32_t gnx_chain_block_forward_narrow_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API size_t gnx_chain_block_forward_narrow_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_chain_block_forward_narrow(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf,
                                       int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out, void* workspace, size_t workspace_bytes,
                                       uint32_t flags, void* stream);
/* Either Chain forward on float32 or bfloat16 features.  `elem` (GNX_ELEM_*) applies to the three feature inputs and the three outputs; weights
 * stay float32.  `narrow` (0 or 1) selects the entry the call mirrors: gnx_chain_block_forward (0) or gnx_chain_block_forward_narrow (1).
 * GNX_ELEM_F32 IS the mirrored entry: same validation, same workspace size, same bits.  Any other elem than F32 / BF16: the call returns
 * GNX_ERR_INVALID_ARG before any GPU work, the queries return 0 (so does a narrow other than 0 / 1).
 * GNX_ELEM_BF16, finite data: the three outputs are bit for bit to_bf16(ref), ref the mirrored fp32 entry on the exactly widened inputs under
 * the same flags, rounded to nearest even once; every intermediate stays fp32.  A bf16 buffer must be 4-byte aligned (else GNX_ERR_INVALID_ARG
 * before any GPU work); rows of odd width and replicas of an odd rows * width then start 2-byte aligned, which is all the kernels assume.
 * Native path — narrow = 1 and every update function that has a non-zero output width AND whose entity has rows is in
 * gnx_chain_block_forward_narrow_applies' mask: each function runs as ONE launch of the fused kernel reading bf16 rows and storing its last
 * layer's row as bf16 (k_chain_mlp_bf16, csrc/gnx_chain_narrow_bf16.hip), under the fp32 entry's profiler names; a function a later one of the
 * call reads also leaves its unrounded fp32 row in the workspace.  Beside those launches only the graph function's helpers run: the widening of
 * gf (G rows) and the materialisation of its input rows.  No edge- or node-sized tensor is widened or rounded by a pass of its own.
 * Workspace: the narrow entry's plus fp32 carves of ef' (if the node or graph function consumes it), nf' (if the graph function does) and
 * the widened gf (if the graph function exists and dg > 0).  _typed_applies: 1 for this path, 0 otherwise (bad arguments and F32 included).
 * Staged path — every other case (narrow = 0, a function outside the rule, a mixed mask): fp32 copies of the three inputs and the three
 * outputs around the mirrored entry; the workspace is that entry's plus the six copies.
 * No class of instantiations is cut from the native rule: see README.md ("Chain blocks on bfloat16 features") for the measured figures.
 * The queries build the handle's tables (call them outside a stream capture); the call allocates nothing, does not synchronise and uses one
 * stream.  Refusals as the mirrored entry's, the workspace one naming gnx_chain_block_forward_typed_workspace_bytes(). */
GNX_API int32_t gnx_chain_block_forward_typed_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t elem, int32_t narrow);
GNX_API size_t gnx_chain_block_forward_typed_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t elem,
                                                             int32_t narrow);
GNX_API int32_t gnx_chain_block_forward_typed(const gnx_graphs* h, const gnx_chain_block_params* p, int32_t elem, const void* ef, const void* nf,
                                              const void* gf, int64_t n_replicas, void* ef_out, void* nf_out, void* gf_out, void* workspace,
                                              size_t workspace_bytes, int32_t narrow, uint32_t flags, void* stream);

/* ---- backward of the block: what a Zygote `rrule` / torch autograd function for (m::GNBlock)(x) needs.
 * Inputs: the forward's inputs (ef, nf, gf), its outputs (ef_out, nf_out, gf_out) and the upstream gradients with the
 * outputs' shapes (g_*; NULL = zero).  Outputs (all optional, NULL = not wanted): gradients w.r.t. the inputs (d_ef, d_nf,
 * d_gf, input shapes) and w.r.t. the parameters (grads->*.weight in the (out x in) column-major layout of the weights,
 * grads->*.bias), OVERWRITTEN.  Deterministic: segmented sums in CSC order, the nf[src] gradient is gathered through a
 * CSR view of the same graph (no atomics), weight gradients are two-stage fixed-order reductions.
 * Activations identity / relu / tanh / sigmoid differentiate from the stored outputs; gelu (not a function of its output) from the
 * pre-activation, recomputed per level. */
typedef struct gnx_dense_grad {
  float* weight; /* (out x in) column-major, device, or NULL */
  float* bias;   /* (out), device, or NULL                   */
} gnx_dense_grad;
typedef struct gnx_block_grads {
  gnx_dense_grad edgefn, nodefn, graphfn;
} gnx_block_grads;
GNX_API size_t gnx_block_backward_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_block_backward(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf, const float* gf,
                           const float* ef_out, const float* nf_out, const float* gf_out, const float* g_ef_out,
                           const float* g_nf_out, const float* g_gf_out, int64_t n_replicas, float* d_ef, float* d_nf,
                           float* d_gf, const gnx_block_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward on bfloat16 feature tensors: the pullback of gnx_block_forward_typed.  `elem` (GNX_ELEM_F32 or GNX_ELEM_BF16) applies to the
 * twelve feature-shaped tensors — the nine inputs and d_ef / d_nf / d_gf; the parameter gradients (gnx_block_grads) stay fp32, as the weights
 * do.  GNX_ELEM_F32 is exactly gnx_block_backward (same validation, same workspace size, same bits); any other `elem` is GNX_ERR_INVALID_ARG
 * before any GPU work, and the workspace query returns 0 for it.  NULL rules, optional outputs, n_replicas rules and status codes are
 * gnx_block_backward's.
 * Contract, for finite data with GNX_ELEM_BF16: with ref = gnx_block_backward on the exactly widened nine inputs, d_ef / d_nf / d_gf are bit for
 * bit to_bf16(ref's) (round to nearest even, once) and every parameter gradient is bit for bit ref's: every intermediate stays fp32 and all
 * sums keep the fp32 backward's fixed orders.
 * This is the fp32 pullback evaluated AT THE ROUNDED SAVED OUTPUTS: ef_out enters the node function's input and act' is taken from the stored
 * (bf16) outputs, not from the unrounded values the forward held in registers.  It is this ABI's convention — the caller supplies the outputs —
 * not a further approximation; a gelu level recomputes its pre-activation in fp32 from the (bf16) inputs.
 * Paths, chosen as gnx_block_backward chooses for the same handle and widths: where neither the edge nor the node level goes to the matrix
 * cores (any widths below 64 rows; README ex.1's widths at every size) the kernels read and write bf16 themselves — no conversion pass, and
 * d_gf, which several launches accumulate, is summed in fp32 in the workspace and rounded once.  Matrix-core widths widen the nine inputs into
 * fp32 regions of the workspace, run gnx_block_backward on them and round the three input gradients.  The workspace is
 * gnx_block_backward_workspace_bytes plus, on the first path, 256-B aligned room for R * G * dg floats, on the second, the twelve fp32
 * copies; the query builds the CSR view and the wide tables, so call it outside any capture.  bf16 buffers must be 4-byte aligned (rows of
 * odd width are then 2-byte aligned: the kernels never assume more) and the workspace 16-byte aligned.  No allocation, no synchronisation. */
GNX_API size_t gnx_block_backward_typed_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API int32_t gnx_block_backward_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const void* ef, const void* nf, const void* gf,
                                         const void* ef_out, const void* nf_out, const void* gf_out, const void* g_ef_out, const void* g_nf_out,
                                         const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf, const gnx_block_grads* grads,
                                         void* workspace, size_t workspace_bytes, void* stream);

/* gnx_block_backward with the edge level of narrow width sets in ONE kernel: a wavefront per wave tile of the handle keeps an edge's input row,
 * its delta and its dXe row in registers — the edge function's input Xe and delta_e are never written, d_ef is written once, and only the
 * 2 dn + dg columns of dXe that d_nf / d_gf sum reach the workspace; the weight / bias gradient of the edge function is summed per tile (edge
 * order), per workgroup (wave order), then by the generic final reduction: fixed orders, no atomics, bitwise reproducible.
 * gnx_block_backward_fused_applies: 1 where the fused edge level runs — (de, dn, dg) => oe one of (10,5,0)=>3, (3,4,5)=>3, (0,2,0)=>2, (2,2,2)=>2,
 * (4,3,2)=>3 (any on / og), E > 0, an edge activation other than gelu, and the edge level not on the matrix cores — else 0 (also for a NULL
 * handle or params).  Where it does not apply, the call IS gnx_block_backward (same bits in every output) and the query returns
 * gnx_block_backward_workspace_bytes.  Where it applies: d_ef, d_nf, d_gf and every node / graph parameter gradient are bit for bit
 * gnx_block_backward's; grads->edgefn.weight / .bias are the same sums in another fixed order.  The workspace has a layout of its own (no Xe, no
 * delta_e, the compact dXe), smaller than the generic one on all but tiny graphs: size it with the fused query.  Arguments, NULL rules,
 * validation and status codes are gnx_block_backward's; buffers need 4-byte alignment only.  No allocation, no synchronisation. */
GNX_API int32_t gnx_block_backward_fused_applies(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas);
GNX_API size_t gnx_block_backward_fused_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_block_backward_fused(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf, const float* gf,
                                 const float* ef_out, const float* nf_out, const float* gf_out, const float* g_ef_out,
                                 const float* g_nf_out, const float* g_gf_out, int64_t n_replicas, float* d_ef, float* d_nf,
                                 float* d_gf, const gnx_block_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The fused narrow edge pullback on bfloat16 feature tensors: gnx_block_backward_typed with the edge level of gnx_block_backward_fused.  `elem`
 * is gnx_block_backward_typed's.  GNX_ELEM_F32: the three entries are gnx_block_backward_fused's.  GNX_ELEM_BF16:
 * gnx_block_backward_fused_typed_applies is 1 where gnx_block_backward_fused_applies is and the typed call is on its native path (neither the
 * edge nor the node level on the matrix cores), else 0; any other `elem` gives 0, and 0 from the workspace query.  Where it does not apply the
 * call IS gnx_block_backward_typed — same validation, same workspace size, same bits.  Where it applies the fused kernel reads ef, nf[src],
 * nf[dst], gf, g_ef_out and ef_out as bfloat16 (widened on load, exact) and writes d_ef as bfloat16 (rounded to nearest even, once); dXe_c, the
 * weight-gradient partial rows and all arithmetic stay fp32.  Contract where it applies, for finite data: d_ef / d_nf / d_gf and the node /
 * graph parameter gradients are bit for bit gnx_block_backward_typed's — and to_bf16 of / equal to gnx_block_backward_fused's on the exactly
 * widened tensors; grads->edgefn.weight / .bias are bit for bit gnx_block_backward_fused's on the widened tensors (the sums of the typed call in
 * another fixed order).  The workspace is the fused layout plus 256-B aligned room for R * G * dg floats (the fp32 sum of d_gf): size it with
 * the query, outside any capture.  Refused before any launch, with gnx_block_backward_typed's statuses: a NULL handle or params, a bad `elem`,
 * bf16 buffers that are not 4-byte aligned, a workspace that is missing or too small. */
GNX_API int32_t gnx_block_backward_fused_typed_applies(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API size_t gnx_block_backward_fused_typed_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API int32_t gnx_block_backward_fused_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const void* ef, const void* nf,
                                               const void* gf, const void* ef_out, const void* nf_out, const void* gf_out, const void* g_ef_out,
                                               const void* g_nf_out, const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf,
                                               const gnx_block_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The fused narrow edge pullback at ANY narrow width set: gnx_block_backward_fused_typed where its five ahead-of-time width sets apply, and the
 * same kernel specialised at run time (hiprtc, as the forward's run-time kernels: gnx_jit_precompile below) for every other eligible set.
 * `elem`, the arguments, NULL rules, status codes and the 4-byte alignment of bf16 buffers are gnx_block_backward_fused_typed's; an unknown
 * `elem` gives 0 from both queries and GNX_ERR_INVALID_ARG from the call.  The call takes one of three forms:
 *  - Ahead-of-time sets: where gnx_block_backward_fused_typed_applies is 1 the call IS gnx_block_backward_fused_typed — same workspace size, same
 *    bits in all nine outputs, grads->edgefn.weight / .bias included.
 *  - Run-time sets: elsewhere the run-time kernel runs when (a) the width set is eligible: oe >= 1, Ke = de + 2 dn + dg >= 1, oe Ke < 64 (the
 *    weight gradient's oe (Ke + 1) pairs fit two per lane) and the kernel's static LDS, 16 (64 ((oe + Ke) | 1) + 64 ceil(oe (Ke + 1) / 64)) bytes,
 *    is within 64 KB (this excludes oe + Ke = 64, e.g. (23,15,10)=>1), with run-time specialisation enabled (not GNX_JIT=0); (b) the other
 *    conditions of the fused call hold: E > 0, wave tiles exist, n_replicas <= 65535 and > 1 only with one graph, an edge activation other than
 *    gelu, the edge level not on the matrix cores, and for GNX_ELEM_BF16 the typed call on its native path; (c) the kernel of this device is
 *    loaded.  Then the workspace is the fused layout (plus the fp32 sum of d_gf for bf16); d_ef, d_nf, d_gf and the node / graph parameter
 *    gradients are bit for bit gnx_block_backward_typed's (gnx_block_backward's for GNX_ELEM_F32); grads->edgefn.weight / .bias are the same
 *    sums in the kernel's fixed order, bitwise reproducible from run to run; and the bf16 call's edge gradients are bit for bit the fp32
 *    narrow call's on the exactly widened tensors.
 *  - Generic: otherwise the call IS gnx_block_backward_typed, with its workspace size and its bits.
 * gnx_block_backward_narrow_applies / _workspace_bytes OBTAIN the kernel of a run-time set — from GNX_JIT_CACHE=<dir> or by compiling it, then
 * loading it on the current device — so they belong outside any capture, like every other query of this header; the first use of a width set
 * costs one hiprtc compilation (a fraction of a second) unless the disk cache holds it.  They answer 1 / the fused size only if the kernel is
 * loaded; loading is sticky per process and device (a failure too), so a call that follows a query takes the form the query announced.
 * A call is never the first to compile inside a capture: a call on a capturing stream for a width set that no query (and no earlier call)
 * loaded finds no kernel, takes the GENERIC form — and refuses a workspace smaller than gnx_block_backward_typed_workspace_bytes with the
 * usual status and message.  Query first, outside the capture.
 * Every class of eligible width sets was measured against the generic call on a 1M-edge graph (profiles/bw_narrow_c2.json: 0.47 - 0.70 of its
 * time, oe = 1 with Ke = 44 and 62 included), so the eligibility rule cuts none out.
 * GNX_JIT_ALL (diagnostic, read once) makes these entries run the run-time kernel at the five ahead-of-time sets too; nothing else changes.
 * gnx_jit_precompile_bw_edge: compile only (no GPU needed; honours GNX_JIT_CACHE) — *code_bytes = size of the code object; GNX_ERR_DIMS for a
 * width set that is not eligible, GNX_ERR_INVALID_ARG for NULL params or a bad `elem`.  Only p->de, dn, dg, oe are read. */
GNX_API int32_t gnx_block_backward_narrow_applies(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API size_t gnx_block_backward_narrow_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API int32_t gnx_block_backward_narrow(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const void* ef, const void* nf,
                                          const void* gf, const void* ef_out, const void* nf_out, const void* gf_out, const void* g_ef_out,
                                          const void* g_nf_out, const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf,
                                          const gnx_block_grads* grads, void* workspace, size_t workspace_bytes, void* stream);
GNX_API int32_t gnx_jit_precompile_bw_edge(const gnx_block_params* p, int32_t elem, size_t* code_bytes);

/* Backward of the Chain block: takes the forward's INPUTS and the upstream gradients (NULL = zero); every layer's output is recomputed
 * into the workspace.  Gradients w.r.t. the inputs (optional) and, per chain, one gnx_dense_grad per layer (host arrays of n_layers
 * entries, or NULL; entries' pointers optional), all OVERWRITTEN.  The tail layers and the node / graph chains are row-wise Dense
 * pullbacks (matrix cores for real matrices), the edge chain's first layer goes through gnx_block_backward; fixed summation orders. */
typedef struct gnx_chain_block_grads {
  const gnx_dense_grad* edgefn;  /* [edgefn.n_layers]  */
  const gnx_dense_grad* nodefn;  /* [nodefn.n_layers]  */
  const gnx_dense_grad* graphfn; /* [graphfn.n_layers] */
} gnx_chain_block_grads;
GNX_API size_t gnx_chain_block_backward_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_chain_block_backward(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf,
                                 const float* g_ef_out, const float* g_nf_out, const float* g_gf_out, int64_t n_replicas, float* d_ef,
                                 float* d_nf, float* d_gf, const gnx_chain_block_grads* grads, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* The same pullback with each update function in ONE kernel where its widths are narrow (k_chain_mlp_bw, csrc/gnx_chain_bw_narrow.hip): a lane
 * builds its row's input as the fused forward does, runs it forward through all layers, forms the last layer's delta (upstream + the shares of
 * the levels above) and walks back through the layers in registers.  The lane's input row and every layer's output but the last wait on a tape
 * in LDS; a gelu pre-activation and a LayerNorm's statistics are recomputed from it.  Parameter gradients are summed per workgroup in a fixed
 * order (no atomics) and finished by one small launch per layer; results are bitwise reproducible and independent of the workspace's contents.
 * The rule is per update function.  With k_in the function's input width and w_i its layer widths (i = 0 .. n - 1), a function is fused when
 *   - gnx_chain_block_forward_narrow's rule takes it (>= 1 layer, w_{n-1} > 0, k_in and every w_i <= 32, staged parameters
 *     par = sum_i (Dense: ceil4(k_i) * ceil4(w_i) + ceil4(w_i); LayerNorm: 2 * ceil4(w_i)) <= 10240 floats, k_0 = k_in, k_i = w_{i-1}; rows), and
 *   - par + 2 * (64 * ld + P) <= 16384 floats (64 KB of LDS for a workgroup of two waves), where
 *       ld = (k_in + sum_{i < n-1} w_i + max_i (Dense: w_i; LayerNorm: 2 * w_i)) | 1     the tape row of a lane (odd),
 *       P  = sum_i (Dense: w_i * (k_i + 1); LayerNorm: 2 * w_i)                          one accumulator per parameter.
 * One wave's tape and accumulators fit 64 KB for every function with all widths <= 16 and <= 8 layers and with all widths <= 32 and <= 3
 * layers, and the kernel runs them; but that one-wave class IS CUT from the rule: measured on the 1M-edge shapes its member (edge [32,32,3] at
 * k_in 23) took 1.34 / 1.75 times the generic pullback's time (profiles/chain_bw_narrow.json).  What stays — e.g. [16,3] at k_in 20,
 * [16,ln,16,3] at k_in 23, [32,4] at k_in 11, eight 8-wide layers — met the bar at all three register widths and source forms.
 * A function the forward fuses and this rule does not is a legitimate mixed case.
 * _applies: bit 0 the edge, bit 1 the node, bit 2 the graph function is fused; 0 on bad arguments (and for an edge function without output,
 * which the call refuses).  _workspace_bytes: a fused function keeps no per-layer outputs, no delta buffers and (the edge function) no inner
 * block workspaces — only what crosses levels (ef', nf', the graph input rows, dXn, dXg), the node / graph columns of the edge rows' input
 * gradient [R E][2 dn + dg] and the partial rows (a fused node function in front of a graph function outside the rule keeps its per-layer
 * outputs: nf' is then recomputed by the generic launches, so that the graph function's parameter gradients keep their bits); it builds the handle's tables the call reads, so call it outside a stream capture (the call
 * itself works inside one).  A function outside the rule runs exactly gnx_chain_block_backward's launches for it; with a mask of 0 the call
 * IS gnx_chain_block_backward (same workspace size, same bits).  Arguments, optional outputs and refusals (in their order) as
 * gnx_chain_block_backward; every buffer may be 4-byte aligned only. */
GNX_API int32_t gnx_chain_block_backward_narrow_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API size_t gnx_chain_block_backward_narrow_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas);
GNX_API int32_t gnx_chain_block_backward_narrow(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf,
                                        const float* g_ef_out, const float* g_nf_out, const float* g_gf_out, int64_t n_replicas, float* d_ef,
                                        float* d_nf, float* d_gf, const gnx_chain_block_grads* grads, void* workspace, size_t workspace_bytes,
                                        void* stream);
/* Either Chain pullback on float32 or bfloat16 features.  `elem` applies to the nine feature-shaped tensors (the inputs, the upstream gradients,
 * the input gradients); parameter gradients stay float32.  `narrow` (0 or 1): gnx_chain_block_backward (0) or gnx_chain_block_backward_narrow
 * (1).  GNX_ELEM_F32 IS the mirrored entry (same validation, workspace size, bits); another elem than F32 / BF16 or a narrow other than 0 / 1:
 * GNX_ERR_INVALID_ARG before any GPU work, 0 from the query.  A bf16 buffer must be 4-byte aligned (GNX_ERR_INVALID_ARG before any GPU work).
 * GNX_ELEM_BF16 is staged here (the bf16 pullback kernel runs behind gnx_chain_block_backward_narrow_typed, below): the six inputs and upstream gradients are widened into fp32 copies (256-byte
 * aligned carves behind the fp32 pullback's workspace), the fp32 pullback runs on them, the three input gradients are rounded back.  d_ef, d_nf,
 * d_gf are bit for bit to_bf16(ref) and every parameter gradient is bit for bit ref's, ref the mirrored fp32 pullback on the exactly widened
 * tensors in 16-byte-aligned buffers.  Optional outputs and NULL upstream gradients as in the fp32 entries.  The workspace is the mirrored
 * entry's plus the nine copies; its refusal names gnx_chain_block_backward_typed_workspace_bytes().  The query builds the handle's tables (call
 * it outside a stream capture); the call allocates nothing, does not synchronise and uses one stream. */
GNX_API size_t gnx_chain_block_backward_typed_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t elem,
                                                              int32_t narrow);
GNX_API int32_t gnx_chain_block_backward_typed(const gnx_graphs* h, const gnx_chain_block_params* p, int32_t elem, const void* ef, const void* nf,
                                               const void* gf, const void* g_ef_out, const void* g_nf_out, const void* g_gf_out, int64_t n_replicas,
                                               void* d_ef, void* d_nf, void* d_gf, const gnx_chain_block_grads* grads, void* workspace,
                                               size_t workspace_bytes, int32_t narrow, void* stream);
/* gnx_chain_block_backward_narrow on float32 or bfloat16 features, bfloat16 NATIVELY where the whole block is narrow (k_chain_mlp_bw_bf16,
 * csrc/gnx_chain_bw_narrow_bf16.hip: k_chain_mlp_bw's body with bf16 feature-shaped operands — the rows gathered and the upstream gradient read
 * with one 16-bit load per element and widened exactly, d_ef rounded to nearest even once and written with one 16-bit store per element; the
 * tape, the accumulators and every arithmetic operation are the fp32 kernel's).  `elem` applies to the nine feature-shaped tensors; parameter
 * gradients stay float32.  The argument list is gnx_chain_block_backward_typed's without `narrow`.
 * The native rule: elem = GNX_ELEM_BF16, the edge function has an output and E > 0, and every update function with a non-zero output width and
 * rows to run on is in gnx_chain_block_backward_narrow_applies' mask.  Then every function is one launch of that kernel on the bf16 rows; ef' and
 * nf' are recomputed by k_chain_mlp_bf16 into the fp32 layout alone; d_nf is summed in the fp32 pullback's order (0, the in-edges, the out-edges,
 * the node function's own share) and rounded once; d_gf accumulates in fp32 and is rounded once.  No E- or N-sized tensor is widened or rounded
 * by a pass of its own: the workspace is gnx_chain_block_backward_narrow's plus two 256-byte-aligned carves of R G dg floats (the widened gf, the
 * fp32 d_gf), and the call launches one k_bf16_widen and one k_bf16_round at the most, both graph-sized (the staged call: six and three).
 * d_ef, d_nf, d_gf and every parameter gradient are bit for bit gnx_chain_block_backward_typed(narrow = 1)'s on the same nine tensors.
 * No class is cut from the native rule (whole calls on the eight shapes of profiles/chain_bw_native.json against the staged call).
 * GNX_ELEM_F32 IS gnx_chain_block_backward_narrow (same validation, workspace size, bits).  GNX_ELEM_BF16 outside the native rule — a mixed
 * mask, no edges — IS gnx_chain_block_backward_typed(narrow = 1) (same workspace size, same bits); a bf16 call's workspace refusal names
 * gnx_chain_block_backward_narrow_typed_workspace_bytes() either way.  _applies: 1 exactly on the native path, 0 otherwise (GNX_ELEM_F32 and bad
 * arguments included).  Another elem than F32 / BF16: GNX_ERR_INVALID_ARG before any GPU work, 0 from the queries.  A bf16 buffer must be
 * 4-byte aligned; optional outputs, NULL upstream gradients and the order of refusals as in gnx_chain_block_backward_typed.  The query builds
 * the handle's tables, the out-edge (CSR) view included — call it outside a stream capture; the call allocates nothing, does not synchronise,
 * uses one stream and works inside a capture. */
GNX_API int32_t gnx_chain_block_backward_narrow_typed_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t elem);
GNX_API size_t gnx_chain_block_backward_narrow_typed_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas,
                                                                     int32_t elem);
GNX_API int32_t gnx_chain_block_backward_narrow_typed(const gnx_graphs* h, const gnx_chain_block_params* p, int32_t elem, const void* ef,
                                                      const void* nf, const void* gf, const void* g_ef_out, const void* g_nf_out,
                                                      const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf,
                                                      const gnx_chain_block_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of (m::GNCore)(x) = x + block(gn1(x)) + ffwd(gn2(x)) (src/gncore.jl:56-68).  Takes the forward's INPUTS and the
 * upstream gradients; the intermediates (both LayerNorms, the block's outputs, the FeedForward hidden activations) are
 * recomputed into the workspace.  Gradient buffers are optional (NULL = not wanted) and overwritten.  FeedForward: fc1 with any
 * activation code (gelu differentiates from the recomputed pre-activation), fc2 with identity (the reference's
 * Chain(Dense(d,4d,relu), Dense(4d,d))). */
typedef struct gnx_layernorm_grad {
  float* gamma;
  float* beta;
} gnx_layernorm_grad;
typedef struct gnx_ffn_grad {
  gnx_dense_grad fc1, fc2;
} gnx_ffn_grad;
typedef struct gnx_core_grads {
  gnx_block_grads block;
  gnx_layernorm_grad ln1[3], ln2[3];
  gnx_ffn_grad ff[3];
} gnx_core_grads;
GNX_API size_t gnx_core_backward_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas);
GNX_API int32_t gnx_core_backward(const gnx_graphs* h, const gnx_core_params* p, const float* ef, const float* nf, const float* gf,
                          const float* g_ef_out, const float* g_nf_out, const float* g_gf_out, int64_t n_replicas, float* d_ef,
                          float* d_nf, float* d_gf, const gnx_core_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward on bfloat16 feature tensors: the pullback of gnx_core_forward_typed.  `elem` (GNX_ELEM_F32 or GNX_ELEM_BF16) applies to the
 * nine feature-shaped tensors — the three inputs, the three upstream gradients and d_ef / d_nf / d_gf; the parameter gradients (gnx_core_grads)
 * stay fp32, as the weights do.  GNX_ELEM_F32 is exactly gnx_core_backward (same validation, same workspace size, same bits); any other `elem`
 * is GNX_ERR_INVALID_ARG before any GPU work, and the workspace query returns 0 for it.  NULL rules, optional outputs, n_replicas rules and
 * status codes are gnx_core_backward's.
 * Contract, for finite data with GNX_ELEM_BF16: with ref = gnx_core_backward on the exactly widened six inputs, every buffer at the same byte
 * offset modulo 16 as in the typed call, d_ef / d_nf / d_gf are bit for bit to_bf16(ref's) (round to nearest even, once) and every parameter
 * gradient is bit for bit ref's.  Nothing is approximate: widening is exact, every intermediate stays fp32 and all sums keep the fp32
 * backward's fixed orders.
 * One path at all widths.  The caller's x is read only by the two LayerNorm kernels that recompute gn1(x) / gn2(x) and by the LayerNorm
 * pullback, which is also the only writer of d_ef / d_nf / d_gf: these kernels take the element type, widen x as they load it and round dx as
 * they store it, so neither x nor an input gradient ever exists as an fp32 tensor.  Each non-NULL upstream gradient is widened once into an
 * fp32 copy behind the fp32 layout of the workspace, which the dW2 sums, the dX products, gnx_block_backward and the pullback's residual read
 * (a NULL one stays NULL).  The kernel forms are chosen as gnx_core_backward chooses them from the caller's addresses: a bf16 x, upstream
 * gradient or d_x that is not 16-byte aligned takes the one-wave-per-row LayerNorm kernels, as a 4-byte aligned fp32 one does.  The workspace
 * is gnx_core_backward_workspace_bytes plus the three 256-B aligned fp32 copies; the query builds the CSR view and the wide tables, so call it
 * outside any capture.  bf16 buffers must be 4-byte aligned (rows of odd width are then 2-byte aligned: the kernels never assume more), else
 * GNX_ERR_INVALID_ARG; the workspace 16-byte aligned, else GNX_ERR_WORKSPACE; both before anything is written or launched.  No allocation, no
 * synchronisation.  With the forward's Dropout active: gnx_core_backward_train_typed. */
GNX_API size_t gnx_core_backward_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem);
GNX_API int32_t gnx_core_backward_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const void* ef, const void* nf, const void* gf,
                                        const void* g_ef_out, const void* g_nf_out, const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf,
                                        void* d_gf, const gnx_core_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* ---- forward: replaces (m::GNCore)(x) (src/gncore.jl:56-68); GNCoreList = caller-side fold (gncorelist.jl:43-45) ----
 * Wide cores (block in the matrix cores' projected form, FeedForward widths 64 / 128): gn1 / gn2 of ef and nf are applied by the
 * kernels as they load x (one pass of row statistics; GNX_FLAG_NO_LN_FUSE materialises the LayerNorms: bit-identical for the node rows and
 * for the two-launch form of the edge rows (GNX_FLAG_CORE_EDGE_SPLIT); the one-launch form of the edge rows carries the LayerNorms' scale
 * in its weight planes and their shift in a constant vector — the same formula in another association, within a few fp32 roundings), and
 * the graph level of the core runs on a side stream (joined before gnx_core_forward returns; part of the capture when `stream` is being
 * captured; GNX_FLAG_NO_FORK: one stream).  The side streams are a small pool of the HANDLE that gnx_core_workspace_bytes creates — call
 * it outside a capture, as every workspace query — and a call holds one only while it enqueues its work.
 * THREADING: a handle is immutable after creation apart from tables built once behind a mutex, so concurrent forwards on ONE handle from
 * several host threads are allowed — each with its own stream, workspace and output buffers (tests/test_gpu_core.py::
 * test_two_host_threads_run_core_forwards_on_one_handle_concurrently: bit-identical to the serial run).  Calls at matrix-core widths (any
 * width above 32) TAKE TURNS ON THE DEVICE: every exported forward / backward holds a per-device lock while it enqueues, waits for the
 * previous such call's end when that ran on another stream, and records an event at its own end (one stream: a lock and an event record
 * per call; a stream under capture is left alone).  Reason (profiles/r05_mfma_mix_hazard.log): on the MI355X boxes this was built on, a
 * kernel on the fp32 matrix instruction returns wrong values now and then — one pass of one instruction: 2 rows x 32 columns — while a
 * dense bf16 matrix kernel runs on another stream of the device, the library's own six-term kernels or anybody else's (a bf16 GEMM);
 * nothing is shared between the two.  GNX_ALLOW_OVERLAP=1 (read once) removes the guard.  Matrix kernels of OTHER libraries that the
 * host runs on other streams beside these calls are the host's to keep apart (an event between the streams).
 * ARITHMETIC of the wide FeedForwards (edges / nodes at width 128 or 64, >= 4096 rows), of the projected edge update at 128 -> 128 or
 * 128 -> at most 32 outputs (gnx_block_forward too, >= 4096 edges) and of its node projections at 64-wide nodes (>= 4096 nodes):
 * fp32 in, fp32 out, fp32 accumulation; every fp32 product is evaluated on the bf16 matrix cores as six terms of an EXACT three-way split
 * of both operands (hi + mid + lo bf16 parts = the 24 mantissa bits; the dropped terms are <= 2^-23 |a||b|) — as accurate as the fp32
 * matrix instruction against float64 by test (tests/test_gpu_x6_stress.py: magnitudes over twelve decades, cancellation, a column scaled by
 * 1e20), 2x its speed; inputs that are not finite (or within 0.4 % of the largest finite float) produce NaN where the fp32 instruction may
 * produce an infinity, and operands below ~1e-33 in magnitude may keep only 16 of their 24 mantissa bits (their low parts are bf16
 * subnormals).  The CALL chooses: GNX_FLAG_FFN_FP32 (FeedForwards) / GNX_FLAG_EDGE_FP32 (edge update and projections) / GNX_FLAG_FP32_MFMA
 * (both) run the kernels on the fp32 matrix instruction instead (csrc/gnx_ffn_fused.hip, csrc/gnx_wide.hip); the environment variables
 * GNX_FFN_FP32 / GNX_EDGE_FP32 set the process-wide default (read once).
 * At 128-wide edges a core's edge update runs inside its edge FeedForward's launch, ef' kept in registers (same bits as two launches:
 * GNX_FLAG_CORE_EDGE_SPLIT), and the row statistics of the edge rows are computed in those kernels (same bits as the statistics pass:
 * GNX_FLAG_LN_STATS_PASS). */
GNX_API size_t gnx_core_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas);
GNX_API int32_t gnx_core_forward(const gnx_graphs* h, const gnx_core_params* p, const float* ef, const float* nf,
                         const float* gf, int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out,
                         void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* The same (test-mode) forward on bfloat16 feature tensors.  `elem` (GNX_ELEM_F32 or GNX_ELEM_BF16) applies to all six tensors; GNX_ELEM_F32
 * is exactly gnx_core_forward (same validation, same workspace size, same bits).  Contract, for finite data with GNX_ELEM_BF16: the three
 * outputs are bit for bit to_bf16(gnx_core_forward(widen(ef), widen(nf), widen(gf))) under the same flags — inputs are widened exactly, every
 * intermediate (gn1 / gn2 rows, the block's three outputs, edge->node sums, graph partial rows, FeedForward hidden units) stays fp32, and
 * only the core's three outputs are rounded, once, to nearest even.  bf16 buffers must be 4-byte aligned (rows of odd width are then 2-byte
 * aligned: the kernels never assume more), else GNX_ERR_INVALID_ARG; the workspace 16-byte aligned, else GNX_ERR_WORKSPACE.
 * Paths.  NATIVE, where the fp32 core runs the fused LayerNorm-on-load block kernel of the ahead-of-time set (README ex.3's widths (10,5,3) at
 * the default wave-tile size, a batch with edges): the same launches as the fp32 core, no conversion pass — the block kernel reads bf16 rows,
 * normalises them on load and hands ef' / nf' / gf' on as fp32 in the workspace (the gn1 regions of the fp32 layout, unused in this form; with
 * the edge FeedForward in the block's edge lanes no edge-sized intermediate exists at all and the core's edge rows are stored as bf16 from
 * there), and k_core_post3 / k_core_post read x as bf16, the block's rows as fp32, and store the core's rows as bf16.  The workspace is
 * gnx_core_workspace_bytes.  FALLBACK, everything else — the matrix-core widths, other narrow triples (run-time specialised ones too),
 * GNX_FLAG_FORCE_GENERIC, GNX_FLAG_NO_JIT, another wave-tile size, a batch without edges: the inputs are widened into fp32 copies behind
 * the fp32 core's workspace, gnx_core_forward runs on them, the outputs are rounded (six fp32 tensors more in the query's size).
 * gnx_core_typed_workspace_bytes sizes the workspace for the path these flags take and warms whatever the call will need (side streams,
 * tables, run-time specialisations), so call it outside any capture; it returns 0 for an unknown `elem` or GNX_FLAG_DEFER_GRAPH_UPDATE with
 * bf16, both of which gnx_core_forward_typed rejects (GNX_ERR_INVALID_ARG) before any GPU work — as it does a misaligned bf16 buffer and
 * (GNX_ERR_DIMS) dims that the block does not map to themselves, each of them even on a NULL handle.  Every other rule is gnx_core_forward's:
 * NULL rules, status codes, no allocation, no synchronisation, capture-safe.  The pullback is gnx_core_backward_typed.  In training mode (an active
 * Dropout): gnx_core_forward_train_typed / gnx_core_backward_train_typed.  Not typed: gnx_model. */
GNX_API size_t gnx_core_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem, uint32_t flags);
GNX_API int32_t gnx_core_forward_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const void* ef, const void* nf, const void* gf,
                                       int64_t n_replicas, void* ef_out, void* nf_out, void* gf_out, void* workspace, size_t workspace_bytes,
                                       uint32_t flags, void* stream);

/* ---- GNCore in TRAINING mode: the Dropout(p) that ends each FeedForward chain (src/gnfeedforward.jl:27-31), applied by Flux inside a
 * gradient call and skipped in test mode (= gnx_core_forward).  y = x + block(gn1(x)) + m .* ffwd(gn2(x)) with m = u > p ? 1/(1-p) : 0,
 * u uniform on [0,1), independent per element (Flux._dropout_kernel).  (GNBlock's own `dropout` field is never applied by its forward:
 * src/gnblock.jl:63-69.)  The masks are never stored: element i of entity t (0 edges, 1 nodes, 2 graphs; i counts the packed
 * [R][rows][width] floats) is a pure function of (seed, t, i) — Philox-4x32-10 — so the backward regenerates the forward's masks from the
 * same gnx_dropout value, and gnx_dropout_mask writes them out for a host that wants to check either pass (tests/test_gpu_dropout.py).
 * (A dropped element therefore holds x + block + (f_fused - f_unfused) — two fp32-accurate evaluations of the same FeedForward, ~1e-6 of its
 * scale apart — not x + block exactly as in Flux; the backward treats its FeedForward gradient as exactly zero.)
 * The host draws a fresh `seed` per forward call (one per core of a GNCoreList).  dropout = NULL or p = 0: exactly gnx_core_forward /
 * gnx_core_backward.  The forward is gnx_core_forward (any flags) followed by the correction y += (m - 1) .* f, f recomputed unfused in the
 * workspace (csrc/gnx_dropout.hip).  The FUSED form of gnx_core_forward_train_typed (below) applies the mask inside the FeedForward kernel and
 * does not carry the (f_fused - f_unfused) residual: a dropped element there is x + block exactly. */
typedef struct gnx_dropout {
  float p;          /* drop probability, 0 <= p <= 1 */
  uint32_t reserved;
  uint64_t seed;
} gnx_dropout;
GNX_API int32_t gnx_dropout_mask(const gnx_dropout* dropout, int32_t entity, int64_t n_elements, float* out, void* stream);
GNX_API size_t gnx_core_train_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas);
GNX_API int32_t gnx_core_forward_train(const gnx_graphs* h, const gnx_core_params* p, const gnx_dropout* dropout, const float* ef, const float* nf,
                               const float* gf, int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out, void* workspace,
                               size_t workspace_bytes, uint32_t flags, void* stream);
/* workspace: gnx_core_backward_workspace_bytes */
GNX_API int32_t gnx_core_backward_train(const gnx_graphs* h, const gnx_core_params* p, const gnx_dropout* dropout, const float* ef, const float* nf,
                                const float* gf, const float* g_ef_out, const float* g_nf_out, const float* g_gf_out, int64_t n_replicas,
                                float* d_ef, float* d_nf, float* d_gf, const gnx_core_grads* grads, void* workspace, size_t workspace_bytes,
                                void* stream);

/* The same backward — (m::GNCore)(x) = x + block(gn1(x)) + ffwd(gn2(x)) (src/gncore.jl:56-59), ffwd = Chain(Dense(d => 4d, relu), Dense(4d => d),
 * Dropout(p)) (src/gnfeedforward.jl:27-31) — with the pullback of each FeedForward in ONE kernel where the core is narrow: a row of gn2(x), its
 * 4d hidden units, their deltas, the upstream gradient and the gradient w.r.t. gn2(x) live in one lane's registers, the weights are scalar
 * operands, and the four weight / bias gradients are summed in the kernel in a fixed order (rows of a 64-row chunk in row order, a wave's chunks in
 * chunk order, a workgroup's waves in wave order, workgroups by the generic finisher) — no atomics, the same bits on every call.  The hidden
 * activations and deltas ([rows][4d], twice) never reach memory, and the workspace carries neither region.
 * gnx_core_backward_narrow_applies = 1: a valid core (dims => dims, all > 0, fc2 identity, valid n_replicas) whose three widths are all within
 * 1..16 and whose three fc1 activations are identity or relu, `elem` GNX_ELEM_F32 or GNX_ELEM_BF16; it does not depend on the row counts.  (No
 * width is cut from the rule: see profiles/core_bw_narrow.json.)  Then every entity with rows and an upstream gradient runs that kernel plus one
 * finisher per Dense; everything else — both LayerNorm passes, the block's forward and pullback, the LayerNorm pullback, the zero fills of an
 * entity without rows or without upstream gradient, the Dropout mask as a pass over the upstream gradient, the bf16 widening — is the launches of
 * gnx_core_backward / _train / _typed.  Results: d_ef, d_nf, d_gf, the block's gradients and the LayerNorm gradients carry the bits of those calls
 * wherever they run their generic kernels (the gradient w.r.t. gn2(x) is computed by the same operations in the same order); the twelve
 * FeedForward gradients are the same sums in another fixed order (a few fp32 roundings apart).
 * `dropout`: NULL or p = 0 — test mode; 0 < p <= 1 with GNX_ELEM_F32 — the pullback of gnx_core_forward_train under the same value; with
 * GNX_ELEM_BF16 an active dropout is GNX_ERR_INVALID_ARG before anything is written (this entry keeps refusing it; the pullback of the typed
 * training-mode forward is gnx_core_backward_train_typed).
 * Where it does not apply, the call IS gnx_core_backward_typed (no active dropout) or gnx_core_backward_train (fp32, active dropout), bit for
 * bit, and the workspace query returns theirs.  The query builds the CSR view and the wide tables: call it outside any capture.  The call
 * itself compiles nothing at run time (sixteen ahead-of-time instantiations cover every core), allocates nothing, does not synchronise and is
 * safe inside a capture.  NULL rules, optional outputs and status codes are gnx_core_backward_typed's; both queries return 0 on a NULL handle or
 * params. */
GNX_API int32_t gnx_core_backward_narrow_applies(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem);
GNX_API size_t gnx_core_backward_narrow_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem);
GNX_API int32_t gnx_core_backward_narrow(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const gnx_dropout* dropout /* NULL: none */,
                                         const void* ef, const void* nf, const void* gf, const void* g_ef_out, const void* g_nf_out, const void* g_gf_out,
                                         int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf, const gnx_core_grads* grads, void* workspace,
                                         size_t workspace_bytes, void* stream);

/* ---- GNCore in TRAINING mode on either element type (src/gncore.jl:56-59, src/gnfeedforward.jl:27-31): y = x + block(gn1(x)) + m .* ffwd(gn2(x))
 * with the masks of gnx_dropout above, on fp32 or bfloat16 feature tensors (`elem` applies to all six), and its pullback.
 * FORWARD.  dropout NULL or p = 0: exactly gnx_core_forward_typed (same bits, same validation, that call's workspace:
 * gnx_core_typed_workspace_bytes).  Active dropout, by path:
 *   FUSED, where gnx_core_train_fused_applies = 1 — the rule of gnx_core_backward_narrow_applies to the letter (the two share one predicate): a
 *   valid core whose three widths are within 1..16, fc1 identity / relu, fc2 identity, `elem` F32 or BF16, independent of the row counts.   No
 *   width is cut from the rule: every measured width is faster than gnx_core_forward_train (profiles/core_train_narrow.json).  Per entity with rows: one gn1 launch (k_ln1_rows, or the same kernel reading
 *   bf16 rows) into the workspace, gnx_block_forward on those rows into fp32 carves of the workspace (the call's `flags` go to the block), then
 *   k_core_post_train (csrc/gnx_core_train_narrow.hip): y = fmaf(m, ffwd(gn2(x)), x + b) with gn2, the 4d hidden units and the mask in one
 *   lane's registers.  No fp32 copy of a bf16 input or output, no hidden units and no f in memory; an entity without rows launches nothing
 *   (ef / ef_out may be NULL when E == 0).  Where m == 0 the element is x + b exactly — the bits of the same call with p = 1.  With
 *   GNX_ELEM_BF16 the outputs are bit for bit to_bf16 of the same entry called with GNX_ELEM_F32 on the exactly widened inputs.
 *   Elsewhere, GNX_ELEM_F32: exactly gnx_core_forward_train (same bits, gnx_core_train_workspace_bytes).  GNX_ELEM_BF16: the three inputs are
 *   widened behind that layout, gnx_core_forward runs in fp32 into fp32 carves, f is recomputed as gnx_core_forward_train does, and one pass
 *   stores to_bf16(fmaf(m - 1, f, y32)) into the caller's buffers: bit for bit to_bf16(gnx_core_forward_train(widened inputs)) under the same
 *   flags and dropout, no value rounded twice.
 * Refused before anything is written or launched, in this order: an unknown `elem` (GNX_ERR_INVALID_ARG), p outside [0, 1]
 * (GNX_ERR_INVALID_ARG), a bf16 buffer that is not 4-byte aligned (GNX_ERR_INVALID_ARG), GNX_FLAG_DEFER_GRAPH_UPDATE with an active dropout
 * (GNX_ERR_INVALID_ARG), dims (GNX_ERR_DIMS), then gnx_core_forward's NULL and parameter rules, a workspace too small or not 16-byte aligned
 * (GNX_ERR_WORKSPACE).  gnx_core_train_typed_workspace_bytes sizes the path an ACTIVE dropout takes; it returns 0 where the call would refuse
 * elem, the handle or the params (and for GNX_FLAG_DEFER_GRAPH_UPDATE), and builds whatever tables that path needs: call it outside a capture.
 * The call allocates nothing, does not synchronise and is capture-safe.  x and y must not overlap.
 * BACKWARD: the pullback of both forward paths under the same gnx_dropout value.  `narrow`: 0 — the launches of gnx_core_backward_train; 1 — those
 * of gnx_core_backward_narrow (k_core_bw_narrow where gnx_core_backward_narrow_applies); anything else is GNX_ERR_INVALID_ARG (the query: 0).
 * With GNX_ELEM_F32 the call IS that entry.  With GNX_ELEM_BF16, ref being that entry on the exactly widened tensors under the same dropout:
 * d_ef / d_nf / d_gf are bit for bit to_bf16(ref's), all parameter gradients bit for bit ref's — the mask is applied to the widened fp32 copy of
 * the upstream gradient.  (gnx_core_backward_narrow itself keeps refusing bf16 with an active dropout.)  Everything else — NULL rules, optional
 * outputs, alignment, status codes, capture — is gnx_core_backward_typed's; the workspace is the size its query returns. */
GNX_API int32_t gnx_core_train_fused_applies(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem);
GNX_API size_t gnx_core_train_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem, uint32_t flags);
GNX_API int32_t gnx_core_forward_train_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const gnx_dropout* dropout, const void* ef,
                                             const void* nf, const void* gf, int64_t n_replicas, void* ef_out, void* nf_out, void* gf_out,
                                             void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);
GNX_API size_t gnx_core_backward_train_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t n_replicas, int32_t elem,
                                                             int32_t narrow);
GNX_API int32_t gnx_core_backward_train_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const gnx_dropout* dropout, int32_t narrow,
                                              const void* ef, const void* nf, const void* gf, const void* g_ef_out, const void* g_nf_out,
                                              const void* g_gf_out, int64_t n_replicas, void* d_ef, void* d_nf, void* d_gf,
                                              const gnx_core_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* ---- GNBlock with Chain update functions in TRAINING mode: `Dropout(p)` layer values inside the chains, e.g.
 * Chain(Dense(a => h, relu), Dropout(p), Dense(h => b)).  GNX_LAYER_DROPOUT is a gnx_chain layer entry: weight = bias = NULL, act = identity, its
 * width = the width of the entry in front of it; it follows a Dense or LayerNorm entry (never first, never behind another Dropout) and may be
 * the last entry.  Only the four *_train entries below take it: gnx_chain_block_forward / _narrow / _typed and the four backward entries refuse
 * it as an unknown layer kind.  fp32 features only.
 * THE MASK is never stored.  Element k of row `row` of replica r of the output of Dropout entry l of function t (0 edge, 1 node, 2 graph; rows
 * = E, N, G; w the entry's width) has the flat index i = (r * rows + row) * w + k and the mask value
 *     m = mask_of(component i % 4 of philox4(i / 4, 16 + 16 t + l, seed), p_l, scale_l),   scale_l = p_l < 1 ? 1 / (1 - p_l) : 0
 * — gnx_dropout_mask's generator on the stream id 16 + 16 t + l (ids 0..2 are GNCore's entities) — and y = x * m is one fp32 multiply.  t and l
 * are indices of the CALLER's chain: where the library puts an identity Dense in front of a LayerNorm-first edge function, and where it drops
 * entries with p = 0, `p` and the stream ids keep the caller's indices.  The backward regenerates the masks from the same record.
 * gnx_chain_dropout_mask writes that mask (for hosts and tests): function 0..2, layer 0..15, p in [0, 1], else GNX_ERR_INVALID_ARG.
 * SEMANTICS.  dropout == NULL, every p_l == 0, or chains without Dropout entries: the call IS the mirrored test-mode entry on the chains with
 * the Dropout entries removed (narrow 0: gnx_chain_block_forward / _backward; 1: _narrow) — same bits, same _applies mask, same workspace
 * size.  An entry with p_l == 0 is removed in any call.  `grads` arrays are indexed by the caller's layers; a Dropout entry's slot is ignored.
 * The two _workspace_bytes queries take no record: they return what a call with EVERY Dropout entry active needs — never less than the mirrored
 * query on the stripped chains, and exactly that for chains without Dropout entries; a call needs what its own record makes of the chains (an
 * identity call: the mirrored entry's size); the workspace refusal of a call with an active entry names the training query.
 * REFUSALS, before any GPU work, in this order: NULL handle or params; a malformed chain (n_layers outside 0..16, NULL layers / widths); a
 * p_l outside [0, 1] (GNX_ERR_INVALID_ARG); a NULL p[t] for a function that has a Dropout entry while dropout != NULL (INVALID_ARG); a
 * misplaced or malformed Dropout entry — first, behind another Dropout, a width other than its input's, an activation, a weight or a bias
 * (INVALID_ARG); narrow other than 0 / 1 (INVALID_ARG); then the mirrored entry's refusals.  The queries return 0 for all of these.
 * GENERIC PATH (narrow = 0, and any function outside the fused rule): a Dropout entry is one k_dropout launch from the layer's input buffer to
 * its output buffer; in the pullback the same launch turns the gradient w.r.t. its output into the gradient w.r.t. its input (no parameter
 * gradient), the delta of the layer in front using that layer's stored, undropped output; a Dropout as last entry multiplies the summed last
 * delta (upstream + the shares of the levels above).
 * FUSED PATH (narrow = 1), per function, with an active Dropout entry counted as a layer of its input's width:
 *   forward rule  : gnx_chain_block_forward_narrow's rule, a Dropout entry counting 0 staged parameter floats (its width <= 32 as any layer's);
 *                   k_chain_mlp_train (csrc/gnx_chain_train_narrow.hip): the lane regenerates the mask of its row in registers, one Philox
 *                   block at a time (a row lies in at most (3 + w + 3) / 4 consecutive blocks; the quad index is 64-bit).
 *   pullback rule : gnx_chain_block_backward_narrow's formula, where a Dropout entry that is not last takes a tape slot of its width like any
 *                   layer output, contributes 0 to par, 0 to P and nothing to the delta slot (the max_i term); two waves per workgroup at
 *                   least, as there.  k_chain_mlp_bw_train (csrc/gnx_chain_bw_train_narrow.hip): k_chain_mlp_bw's text with the Dropout op —
 *                   the dropped row goes on the tape, the way back multiplies the gradient by the regenerated mask; no accumulators, no
 *                   parameter-gradient phase for the entry.
 *                   ONE CLASS IS CUT from the pullback's rule: an EDGE function with Dropout entries at register width 32 (k_in or a layer
 *                   width beyond 16) — its kernel takes 256 VGPRs, and both measured cases ([16,do,3] at k_in 20: 2.02 against 1.02 ms on the
 *                   1M-edge batch, 5.18 against 4.16 ms on one 1M-edge graph) were slower than the generic test-mode pullback beyond its spread
 *                   (profiles/chain_train_narrow.json).  Such a function runs the generic training launches.  No class is cut from the
 *                   forward's rule (0.42 - 1.00 of the generic test-mode forward on the eight measured cases).
 * No new instantiation uses scratch (profiles/chain_train_narrow_resources.json).  A function without an active Dropout entry runs the
 * test-mode kernels under the test-mode rules.  ef' / nf' that cross levels are recomputed in the pullback by the training forward kernel under
 * the same record; mixed masks and a fused node function in front of a generic graph function behave as in the test-mode entries; the
 * workspace of a fused function is what it is there.  Results of a fused function: the forward's bits are those of the generic launches' operations in
 * layer order as for gnx_chain_block_forward_narrow (within 1e-5 of the generic path, not its bits); the masks are the same bits on both paths.
 * gnx_chain_block_train_applies(h, p, R, backward): the fused mask of the training rule (bit 0 edge, 1 node, 2 graph) of the forward
 * (backward = 0) or the pullback (1) for chains whose Dropout entries are all active; 0 on bad arguments.  Without Dropout entries it equals
 * gnx_chain_block_forward_narrow_applies / gnx_chain_block_backward_narrow_applies.
 * The calls allocate nothing, do not synchronise, use one stream and work inside a capture (the seed travels by value); the queries build the
 * handle's tables: call them outside a capture. */
#define GNX_LAYER_DROPOUT 2
typedef struct gnx_chain_dropout {
  uint64_t seed;     /* fresh per forward call; the backward gets the same value */
  const float* p[3]; /* edge / node / graph function: host array [n_layers] or NULL; entry i is read only where layer i is GNX_LAYER_DROPOUT */
} gnx_chain_dropout;
GNX_API int32_t gnx_chain_dropout_mask(const gnx_chain_dropout* dropout, int32_t function, int32_t layer, float p, int64_t n_elements, float* out,
                                       void* stream);
GNX_API int32_t gnx_chain_block_train_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t backward);
GNX_API size_t gnx_chain_block_forward_train_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t narrow);
GNX_API int32_t gnx_chain_block_forward_train(const gnx_graphs* h, const gnx_chain_block_params* p, const gnx_chain_dropout* dropout, const float* ef,
                                              const float* nf, const float* gf, int64_t n_replicas, float* ef_out, float* nf_out, float* gf_out,
                                              void* workspace, size_t workspace_bytes, int32_t narrow, uint32_t flags, void* stream);
GNX_API size_t gnx_chain_block_backward_train_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t n_replicas, int32_t narrow);
GNX_API int32_t gnx_chain_block_backward_train(const gnx_graphs* h, const gnx_chain_block_params* p, const gnx_chain_dropout* dropout, const float* ef,
                                               const float* nf, const float* gf, const float* g_ef_out, const float* g_nf_out, const float* g_gf_out,
                                               int64_t n_replicas, float* d_ef, float* d_nf, float* d_gf, const gnx_chain_block_grads* grads,
                                               void* workspace, size_t workspace_bytes, int32_t narrow, void* stream);

/* ---- row statistics of a packed [rows][d] tensor: stats[row] = (mean, 1 / (sigma + eps)) (eps_mode 0, Flux 0.14 `normalise`) or
 * (mean, 1 / sqrt(sigma^2 + eps)) (eps_mode 1), uncorrected sigma — the one pass over x from which the wide kernels apply GNGraphNorm's
 * LayerNorms (src/gngraphnorm.jl:19-26) as they load their rows; exported as the building block it is (and so that it can be exercised
 * on its own: tests/overlap_probe.py).  d must be a multiple of 64 up to 512; x and stats [rows][2] 4-byte aligned as every fp32 buffer (the
 * same bits at any alignment). */
GNX_API int32_t gnx_row_stats(const float* x, int64_t rows, int32_t d, float eps, int32_t eps_mode, float* stats, void* stream);

/* ---- materialised update-function inputs: the reference's exported building blocks getedgefninput /
 * getnodefninput / getgraphfninput (src/edgefninput.jl:1-47, src/nodefninput.jl:1-24, src/graphfninput.jl:1-13).
 * The forward never materialises them; these exist for callers that use the building blocks directly.
 *   kind 0 (edge):  out [R][E][de+2dn+dg] = [ef ; nf[src] ; nf[dst] ; gf[g]]
 *   kind 1 (node):  out [R][N][de+dn+dg]  = [sum_{e->n} ef ; nf ; gf[g]]        (ef = the UPDATED edge features)
 *   kind 2 (graph): out [R][G][de+dn+dg]  = [sum_e ef ; sum_n nf ; gf]
 * A width of 0 / a NULL pointer drops that segment exactly like the `nothing` methods of the reference. */
GNX_API int32_t gnx_fn_input(const gnx_graphs* h, int32_t kind, const float* ef, int32_t de, const float* nf, int32_t dn,
                     const float* gf, int32_t dg, int64_t n_replicas, float* out, void* stream);

/* ---- edge collapsing: unpaddedcollapsedef / flatunpaddedcollapsedef (src/gngraphbatch.jl:56-111, exported at
 * src/GraphNets.jl:50; reference tests test/runtests.jl:4-59).  For every real edge i->j with i >= j (the lower
 * triangle of the adjacency matrix, in edge order) the symmetric average (ef[i->j] + ef[j->i]) / 2; a self loop gives
 * ef[i->i].  If the reverse edge does not exist it contributes 0 (the reference reads the padded slot there, which is
 * 0 for batched inputs and junk for block outputs).
 * gnx_collapse_offsets: off[G+1] = per-graph offsets into the collapsed rows (off[G] = total).
 * gnx_collapse_edges:   out [R][total][d] from ef [R][E][d]. */
GNX_API int32_t gnx_collapse_offsets(const gnx_graphs* h, int64_t* off);
GNX_API int32_t gnx_collapse_edges(const gnx_graphs* h, const float* ef, int32_t d, int64_t n_replicas, float* out, void* stream);
/* collapsef itself (src/gngraphbatch.jl:83-85: batched_mul(ef, edge_collapser) / 2 with the collapser of :67-82), the PADDED array
 * form: out [B][L][d], B = graphs of the batch (or n_replicas of a shared graph), L = PN(PN+1)/2 coordinates (i, j), i >= j, of the
 * padded PN x PN grid in column-major order; out[b][l] = (P[i->j] + P[j->i]) / 2 over the zero-padded edge grid P (P[i->i] on the
 * diagonal).  = Julia (d, L, B).  The reference reads whatever its padded array holds in non-edge slots; here they are 0. */
GNX_API int32_t gnx_collapse_padded(const gnx_graphs* h, const float* ef, int32_t d, int64_t n_replicas, float* out, void* stream);

/* ---- readout loss on packed outputs: Flux.logitcrossentropy(yhat, y) over the columns of
 * flatunpaddednf / flatunpaddedef, as used by the reference's only end-to-end workload (examples/sort/sort.jl:69-81):
 *   loss = mean over columns c of  -sum_k y[k,c] * logsoftmax(yhat[:,c])[k]
 * logits / targets: device [cols][d] rows (= Julia (d, cols) column-major); loss_out: ONE device float.
 * workspace: gnx_xent_workspace_bytes(cols) bytes.  Deterministic two-stage reduction. */
GNX_API size_t gnx_xent_workspace_bytes(int64_t cols);
GNX_API int32_t gnx_logit_cross_entropy(const float* logits, const float* targets, int32_t d, int64_t cols, float* loss_out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* pullback of gnx_logit_cross_entropy w.r.t. the logits: d_logits[c][k] = g * (sum_k' y[k',c] * softmax(yhat[:,c])[k] - y[k,c]) / cols,
 * g = *upstream (ONE device float, the gradient of the scalar loss) */
GNX_API int32_t gnx_logit_cross_entropy_backward(const float* logits, const float* targets, int32_t d, int64_t cols,
                                         const float* upstream, float* d_logits, void* stream);

/* ---- reference-layout bridges: padef/padnf and unpadef/unpadnf (src/pad.jl:12-64, src/unpad.jl:1-17) ----
 * kind 0 = edges: packed [R][E][d] <-> padded [B][PN^2][d];  kind 1 = nodes: packed [R][N][d] <-> padded [B][PN][d],
 * where B = R (one graph in the handle) or G (R must be 1).  Pads are written as zeros.  `packed` may be NULL for a batch
 * without edges (E = 0: padef gives an array of zeros, unpadef writes nothing). */
GNX_API int32_t gnx_pad_features(const gnx_graphs* h, int32_t kind, const float* packed, int32_t d, int64_t n_replicas,
                         float* padded, void* stream);
GNX_API int32_t gnx_unpad_features(const gnx_graphs* h, int32_t kind, const float* padded, int32_t d, int64_t n_replicas,
                           float* packed, void* stream);

/* ---- a list of layers as ONE hipGraph: replaces a host-side chain such as the reference's
 *      `decoder(core(encoder(x)))` (examples/sort/sort.jl:68-75; GNCoreList is a foldl, src/gncorelist.jl:43-45) ------------
 * At README-sized widths a layer is ~25 us of GPU work, less than the host spends launching it: a multi-layer model is
 * launch-bound.  gnx_model_create copies the layer descriptors (NOT the weights: the device pointers inside stay the
 * caller's and must stay valid), sizes every intermediate tensor and workspace once (library-owned device memory, freed by
 * gnx_model_destroy) and compiles any run-time specialised kernel.  gnx_model_forward runs the layers back to back on
 * `stream`; the first call with a given set of input/output pointers captures them into a hipGraph (on an internal stream),
 * later calls with the same pointers replay it with one hipGraphLaunch (new pointers: re-capture) — unless the captured forward is fewer
 * than five kernels (one narrow GNBlock: two), which is launched kernel by kernel: faster than a replay's launch latency (24.9 vs 29.9
 * us/step on BASELINE configs[1]; env GNX_MODEL_GRAPH_MIN_NODES).  GNX_FLAG_NO_GRAPH runs
 * eagerly.  Layer i's output widths must equal layer i+1's input widths (GNX_ERR_DIMS).  One forward at a time per model. */
typedef struct gnx_model gnx_model;
#define GNX_LAYER_BLOCK 0
#define GNX_LAYER_CORE 1
typedef struct gnx_layer {
  int32_t kind;       /* GNX_LAYER_BLOCK: params -> gnx_block_params; GNX_LAYER_CORE: params -> gnx_core_params */
  int32_t reserved;
  const void* params;
} gnx_layer;
#define GNX_FLAG_NO_GRAPH 0x8u
GNX_API int32_t gnx_model_create(const gnx_graphs* h, const gnx_layer* layers, int32_t n_layers, int64_t n_replicas, gnx_model** out);
GNX_API int32_t gnx_model_destroy(gnx_model* m);
/* widths of the model's output (DE', DN', DG'); 0 <=> nothing */
GNX_API int32_t gnx_model_out_dims(const gnx_model* m, int32_t dims[3]);
GNX_API int32_t gnx_model_forward(gnx_model* m, const float* ef, const float* nf, const float* gf, float* ef_out, float* nf_out,
                          float* gf_out, uint32_t flags, void* stream);
/* gnx_model_create prepares the parameters of every layer whose descriptor carries no `prepared` object (the model owns those objects).
 * After the weights' VALUES changed (an optimiser step; same pointers) call this before the next gnx_model_forward. */
GNX_API int32_t gnx_model_refresh_weights(gnx_model* m, void* stream);

/* ---- multi-GPU: whole graphs sharded over the devices of ONE host process, gf' all-gathered ------------
 * The reference has no multi-device code (nothing to cite in /root/reference/src); the contract is BASELINE.json's north_star:
 * "heterogeneous-graph batches shard by graph across the 8 GPUs of one node with RCCL all-gather of graph-level features".
 * Every term of a graph's edge, node and graph update depends on that graph only, so a rank needs nothing from another rank:
 * it builds a gnx_graphs handle of ITS graphs (gnx_graphs_create_*) and keeps its ef / nf / gf rows resident; the only
 * collective is one all-gather of gf'.  One process drives all devices (ncclCommInitAll, ncclGroupStart/End), which is how a
 * Julia session uses a multi-GPU node.  RCCL is loaded at run time (librccl.so.1).
 *
 * gnx_dist_partition (host only): equal graph counts per rank (+-1), balanced by edge count — graphs sorted by E_g descending
 * (ties: ascending id), dealt to ranks in snake order 0..R-1, R-1..0, ...; rank r owns the original graph ids
 * shard_graphs[shard_off[r] .. shard_off[r+1]), ascending.  shard_off has n_ranks+1 entries, shard_graphs n_graphs.
 * gnx_dist_create: communicator over device_ids[0..n) plus the gather plan of a partition (any permutation of the graphs:
 * rank r's local handle holds its graphs in the order they appear in shard_graphs) for gf' rows of `og` floats.
 * gnx_dist_allgather_gf: gf_local[r] = device-r rows [count_r][og] of rank r's graphs; afterwards gf_all[r] = device-r table
 * [n_graphs][og] in ORIGINAL graph order on every rank.  streams[r] (NULL array / entry = default stream): the stream of
 * device r that produced gf_local[r]; the collective runs on internal streams behind it and gf_all[r] is ready on it.
 * gnx_dist_block_forward: per rank gnx_block_forward(h[r], p[r], ...; n_replicas = 1) on device r (parameters replicated by
 * the caller: p[r] points at device-r copies), then the all-gather of gf'.  Arrays have one entry per rank. */
typedef struct gnx_dist gnx_dist;
GNX_API int32_t gnx_dist_partition(const int64_t* edge_counts, int64_t n_graphs, int32_t n_ranks, int64_t* shard_off, int64_t* shard_graphs);
GNX_API int32_t gnx_dist_create(const int32_t* device_ids, int32_t n_devices, const int64_t* shard_off, const int64_t* shard_graphs,
                        int64_t n_graphs, int32_t og, gnx_dist** out);
GNX_API int32_t gnx_dist_destroy(gnx_dist* d);
/* the gather plan of a partition, on the host (no device, no RCCL): validates shard_off / shard_graphs (a permutation of the graphs)
 * and writes src_row[g] = row of original graph g in the gathered [n_ranks * max_count][og] table (every rank contributes max_count rows,
 * zero padded).  gnx_dist_create builds its plan with this function.  src_row / max_count may be NULL. */
GNX_API int32_t gnx_dist_gather_plan(const int64_t* shard_off, const int64_t* shard_graphs, int32_t n_ranks, int64_t n_graphs, int32_t* src_row,
                             int64_t* max_count);
/* out[g][:] = gathered[src_row[g]][:] on the device (all three device pointers): the permutation back to ORIGINAL graph order that
 * follows the all-gather, for hosts that run the collective themselves (one process per GPU over torch.distributed / MPI) */
GNX_API int32_t gnx_dist_permute_rows(const float* gathered, const int32_t* src_row, int64_t n_graphs, int32_t og, float* out, void* stream);
GNX_API int32_t gnx_dist_allgather_gf(gnx_dist* d, const float* const* gf_local, float* const* gf_all, void* const* streams);
GNX_API int32_t gnx_dist_block_forward(gnx_dist* d, const gnx_graphs* const* h, const gnx_block_params* const* p, const float* const* ef,
                               const float* const* nf, const float* const* gf, float* const* ef_out, float* const* nf_out,
                               float* const* gf_out_local, float* const* gf_all, void* const* workspace, const size_t* workspace_bytes,
                               uint32_t flags, void* const* streams);

/* The replay form of the sharded forward, for loops over many batches of the same graphs (training / serving): n_steps block forwards
 * per rank — independent batches: step s of rank r reads ef / nf / gf [s * n_ranks + r] and writes ef_out / nf_out [s * n_ranks + r] with the
 * workspace [s * n_ranks + r] of workspace_bytes[r] bytes — whose gf' rows go straight into the communicator's stacked send buffer; ONE grouped
 * all-gather moves the n_steps tables of every rank and gf_all[r] (device r) receives [n_steps][n_graphs][og] in ORIGINAL graph order.
 * h / p / workspace_bytes / gf_all / streams have one entry per rank.  The launch sequence of a rank is captured into ONE hipGraph per
 * device the first time a set of arguments is seen (that call runs eagerly and captures; up to 32 argument sets are kept per communicator)
 * and replayed with one hipGraphLaunch per device afterwards: the host issues n_ranks graph launches + one grouped collective + n_ranks
 * permute kernels per call, whatever n_steps is.  GNX_FLAG_NO_GRAPH: always eager.  One call at a time per communicator.
 * An argument set is identified by what the captured launches contain: every pointer, the handles' identities (a serial number, not
 * the address) and the CONTENTS of *p[r] — a descriptor rewritten in place, or a handle destroyed and recreated at the same address, is
 * a new set.  GNX_FLAG_DIST_NO_GATHER: the forwards only (no collective, gf_all untouched) — what the all-gather costs is the difference. */
#define GNX_FLAG_DIST_NO_GATHER 0x10u
GNX_API int32_t gnx_dist_block_forward_steps(gnx_dist* d, int32_t n_steps, const gnx_graphs* const* h, const gnx_block_params* const* p,
                                     const float* const* ef, const float* const* nf, const float* const* gf, float* const* ef_out,
                                     float* const* nf_out, float* const* gf_all, void* const* workspace, const size_t* workspace_bytes,
                                     uint32_t flags, void* const* streams);

/* ---- run-time specialisation (the analogue of Julia compiling a GNBlock for its own widths on first use) -----------
 * The fused one-launch kernel is compiled ahead of time for the README / benchmark width sets; for any other width set
 * with every width <= 32 (and at most 1024 weights in the edge and node functions) it is compiled at run time with hiprtc (gfx950), once per process and device, the first time
 * gnx_block_workspace_bytes / gnx_block_forward sees the width set (never while the stream is being captured: such a
 * call runs the generic kernels).  GNX_JIT=0 disables it; GNX_JIT_CACHE=<dir> keeps the code objects on disk.
 * If hiprtc is unavailable the generic HIP kernels run instead.
 * gnx_jit_precompile: compile only (no GPU needed) — build-time / CI check; *code_bytes = size of the code object.
 * gnx_jit_stats: out = {compiled, disk-cache hits, failures, first uses inside a capture}. */
GNX_API int32_t gnx_jit_precompile(const gnx_block_params* p, int32_t wtile_e_cap, size_t* code_bytes);
/* the same check for the one-launch FeedForward + residual kernel of a narrow GNCore (widths 1..16), which is specialised at run time for
 * width triples other than README ex.3's (10,5,3) */
/* gnx_jit_precompile for the kernel of another element type of the feature tensors (GNX_ELEM_F32: gnx_jit_precompile; GNX_ELEM_BF16) */
GNX_API int32_t gnx_jit_precompile_typed(const gnx_block_params* p, int32_t wtile_e_cap, int32_t elem, size_t* code_bytes);
GNX_API int32_t gnx_jit_precompile_core_post(int32_t de, int32_t dn, int32_t dg, size_t* code_bytes);
GNX_API int32_t gnx_jit_stats(int64_t out[4]);

/* ---- per-kernel timing from dispatch timestamps (bench / roofline evidence): while enabled, every kernel the library launches carries a
 * start / stop event pair on its own dispatch packet (hipExtLaunchKernel) — the kernel's begin -> end as rocprofv3's kernel trace reports
 * it, plus a constant ~3.9 us that gnx_profile_calibrate measures on an empty kernel ---- */
GNX_API int32_t gnx_profile_enable(int32_t on);
GNX_API int32_t gnx_profile_reset(void);
/* n launches of an empty kernel timed the same way (entry "__empty_bracket__"): the constant of the method */
GNX_API int32_t gnx_profile_calibrate(int32_t n, void* stream);
/* synchronises the recorded events; writes up to `max` entries, returns how many exist in *n */
GNX_API int32_t gnx_profile_read(gnx_profile_entry* out, int32_t max, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* GNX_H */
