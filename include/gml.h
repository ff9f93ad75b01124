/*
 * gml.h -- C ABI of libgml_hip.so: the MI355X (gfx950) kernels behind the GNNML1/GNNML3
 * spectral layer (SpectConv / ML3Layer of balcilar/gnn-matlang).
 *
 * Conventions
 *   - every entry point returns int: 0 = ok, >0 = hipError_t, <0 = GML_E_* argument error;
 *   - no allocation, no global state, no synchronisation inside: the caller owns every buffer
 *     (device pointers), passes the hipStream_t the work is ordered on, and sizes scratch with
 *     the *_workspace_bytes helpers;
 *   - all matrices are row-major fp32 with an explicit leading dimension in ELEMENTS;
 *     node ids / edge positions are int32 on the device (int64 only at the COO boundary, which
 *     is what the reference hands over);
 *   - inputs are never written.
 *
 * What each entry replaces in the reference (pure Python, so the "FFI" a maintainer binds is
 * ctypes -- see INTEGRATION.md):
 *   gml_csr_*            nothing (the reference hands edge_index [2,E] int64 straight to PyG
 *                        MessagePassing.propagate, libs/spect_conv.py:77); the CSR keeps PyG's
 *                        per-target summation order (stable in input-edge order)
 *   gml_spectconv_fwd    SpectConv.forward default branch, libs/spect_conv.py:68-80,93-96 +
 *                        message :98-99 + PyG propagate (gather, scale, scatter-add) + matmul
 *   gml_spmm_fwd         the S propagate() calls alone (libs/spect_conv.py:77): H_s = A_s^T X
 *   gml_sddmm            autograd of message() w.r.t. norm (libs/spect_conv.py:98-99)
 *   gml_edge_mlp_*       ML3Layer.forward edge branch, libs/spect_conv.py:205-207
 *   gml_node_mix_*       ML3Layer.forward Hadamard branch, libs/spect_conv.py:209 (tanh*tanh)
 *   gml_relu_bwd / gml_segment_sum   glue the fused layer needs around the above
 */
#ifndef GML_H_
#define GML_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gml_stream_t; /* hipStream_t */

enum {
    GML_OK = 0,
    GML_E_BADARG = -1,       /* null pointer / negative size / bad stride */
    GML_E_UNSUPPORTED = -2,  /* shape outside the compiled kernel set */
    GML_E_WORKSPACE = -3     /* workspace too small */
};

/* flags of gml_spectconv_fwd */
enum {
    GML_RELU = 1,   /* out = max(out, 0) in the epilogue          (ML3Layer: relu(conv1(..))) */
    GML_ACCUM = 2,  /* out += result instead of out = result      (gradient accumulation)     */
    GML_F32_MFMA = 4, /* project with the f32-input MFMA (bit-identical to an fmaf chain) instead of the default
                         bf16x3 split on the bf16 matrix cores (fp32-class: ~1e-6 of the output scale)       */
    GML_GROUPS128 = 8, /* gml_spectconv_fwd: `ginfo` holds 128-row group records (gml_spectconv_fwd_group_rows() = 128):
                         the 8-wave forward kernel                                                            */
    /* 16: unused (was GML_GROUPS64R, the 8-wave kernel's 4-wave geometry on ranked 64-row records; removed, 5a81d54 is the last
                         commit that has it) */
    GML_FWD_CHUNKED = 64, /* gml_spectconv_fwd / gml_ml3_fwd with GML_GROUPS128: some 128-row group holds more edges than the ring
                         kernel stages at once (the caller knows the maximum from its group records): take the chunked ring kernel
                         (gml_k_spectconv_fwd4), which walks such groups in edge chunks instead of gathering from global memory */
    GML_DVAL_ACCUM = 128, /* gml_spectconv_bwd (8-wave bf16x3 kernel): dval += instead of dval = -- the second of two launches over
                         slices of the input features (48-wide layers: features 0..31, then 32..47; dval is linear in x).
                         GML_E_UNSUPPORTED where the selected kernel has no such copy-out: the 64-row kernel, S = 8 with 17 .. 32 output
                         columns, and 33 .. 48 input features in one launch */
    GML_FWD_ONEWIN = 256, /* gml_spectconv_fwd, 48-feature shapes on the chunked ring kernel: ONE staged X window instead of two, twice the
                         edges per work item -- for batches whose groups need edge chunks (the caller knows the batch's largest group) */
    GML_DMA_RING = 32,  /* gml_spectconv_bwd / _bwd_mix: take the LDS-DMA landing-ring kernel (bwd4) where it applies; the
                         forward uses its ring kernel (fwd3) by default                                                  */
    GML_F16X3 = 1024,   /* gml_spectconv_fwd / gml_ml3_fwd on the 8-wave kernels (fwd3, its register-staged form fwd2, the chunked ring kernel fwd4): project with f16 (hi, lo) pieces under per-tile /
                         per-column power-of-two scales instead of bf16 pairs: residual 2^-24 instead of 2^-17 per operand, same
                         instruction count on the matrix pipe (csrc/gml_common.h "f16x3").  Ignored by the 64-row kernel family. */
    GML_NO_FOLD = 512   /* gml_spectconv_bwd / _bwd_mix / _bwd_mix_relu with dw != NULL: dw is NOT written -- the per-workgroup partial
                         sums stay in ws as [parts][S * Fin * Fout], parts = gml_spectconv_bwd_workspace_bytes(...) / (4 S Fin Fout) --
                         for a later gml_fold_many (the reference's batch 64: twelve fold launches of a step become one) */
};

/* gml_spectconv_bwd_mix_relu with the rows of wmix in two arrays (rows [0, nmix_a) from wmix_a, the next nmix_b from wmix_b): an
 * ML3Layer's fc11.weight and fc12.weight as they are stored -- no concatenation launch per layer and step. */
int gml_spectconv_bwd_mix_relu2(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const float* val,
                                const float* x, int64_t ldx, const float* g, int64_t ldg, const float* w,
                                float* dx, int64_t lddx, float* dval, float* dw, const float* dz, const float* wmix_a,
                                int32_t nmix_a, const float* wmix_b, int32_t nmix_b, int32_t relu_cols, int64_t num_rows,
                                int32_t S, int32_t Fin, int32_t Fout, int32_t max_group_edges, int32_t max_group_window,
                                uint32_t flags, void* ws, size_t ws_bytes, gml_stream_t stream);

/* gml_spectconv_bwd_mix_relu2 with the whole output stage of the ML3Layer inside -- the backward of
 *   out = cat[ relu(conv(x)) , tanh(fc11 x) * tanh(fc12 x) ]          (libs/spect_conv.py:209-212)
 * for a layer whose output gradient arrives pre-masked (the consumer layer's conv backward applied this layer's relu mask,
 * relu_cols above): ONE launch instead of gml_ml3_split_bwd_ex + gml_spectconv_bwd_mix_relu2.  g [num_rows, ldg >= Fout + F2] is
 * that gradient (columns [0, Fout) at the conv output, columns Fout, Fout + 1 at the Hadamard units); neither a dz array nor a second
 * pass over g and x exists -- dz is recomputed per 128-row group from the x rows the kernel holds, dw11 / dw12 ride in the kernel's own
 * row contraction (bf16x3 products like dw), the bias gradients are folded per wave in fixed order.  Shape class: S = 8,
 * 17 .. 32 input features (multiple of 4), Fout = 30, F2 = 2 (Zinc12k.py:338-341); gml_spectconv_bwd_had_parts returns 0 outside it
 * (and with GML_BWD_HAD=0 in the environment), otherwise the number of partial rows [dw11 | dw12 | db11 | db12 | dcb]
 * (4 Fin + 4 + Fout floats each) hws must hold.  dcb = dw11 = db11 = dw12 = db12 = NULL: the partials stay in hws for gml_fold_many;
 * otherwise they are folded into the given ones (dw11, dw12 required then; b11 / db11, b12 / db12 may be NULL).  dw required.
 * dx = NULL (want_dx = 0; the model's first layer, whose input is data): no dX is formed; then 17 .. 32 input features of any count,
 * x rows float4-readable up to roundup4(Fin) (ldx % 4 == 0, 16-byte aligned base), relu_cols = 0. */
int gml_spectconv_bwd_had_parts(int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout, int32_t F2, int32_t want_dx,
                                int32_t max_group_edges, int32_t max_group_window, uint32_t flags);
int gml_spectconv_bwd_had(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const float* val,
                          const float* x, int64_t ldx, const float* g, int64_t ldg, const float* w,
                          float* dx, int64_t lddx, float* dval, float* dw, const float* w11, const float* b11,
                          const float* w12, const float* b12, int32_t relu_cols, float* dcb, float* dw11, float* db11,
                          float* dw12, float* db12, int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout, int32_t F2,
                          int32_t max_group_edges, int32_t max_group_window, uint32_t flags, void* ws, size_t ws_bytes,
                          void* hws, size_t hws_bytes, gml_stream_t stream);

/* Deferred folds.  Every weight-gradient kernel of the library leaves one partial sum per workgroup in its workspace and folds
 * them in a second launch.  At the reference's batch size those folds are launches of a few microseconds of work each; a caller
 * may skip them -- GML_NO_FOLD above; gml_ml3_split_bwd(_ex) with dcb = dw11 = db11 = dw12 = db12 = NULL (partials [parts][2 F2 Fin +
 * 2 F2 + nout1] in the order dw11, dw12, db11, db12, dcb; parts = gml_ml3_split_bwd_workspace_bytes / row bytes); gml_edge_mlp_bwd
 * with dw1 = dw2 = dw3 = dw4 = NULL (partials [gml_edge_mlp_bwd_parts(...)][6 S^2 + 4 S Sout] in the order dw1..dw4) -- and fold all
 * of them with ONE launch:  dst[k][i] = sum_{w < nparts} partial[w * n + off_k + i]  in ascending w (the order of the per-kernel
 * folds: bit-identical results), off_k = ndst[0] + .. + ndst[k-1]; a NULL dst[k] skips its segment. */
typedef struct gml_fold_job {
    const float* partial; int64_t nparts; int64_t n;
    float* dst[5]; int64_t ndst[5];
} gml_fold_job;
#define GML_FOLD_MAX_JOBS 16
int gml_fold_many(const gml_fold_job* jobs /* host array */, int32_t njobs /* <= GML_FOLD_MAX_JOBS */, gml_stream_t stream);
/* Adam (torch.optim.Adam's update as the reference scripts configure it, Zinc12k.py:349: no weight decay, no amsgrad) over a list of
 * tensors in ONE launch: t = step[0] + 1; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) m / (sqrt(v / (1 - b2^t)) + eps);
 * step[0] = t afterwards.  step [1] fp32 and done [1] uint32 (zero) live on the device: the launch is capturable, every replay of a
 * captured step advances the count.  More than GML_ADAM_MAX_JOBS tensors: several calls -- all but the last with a scratch copy of
 * step (the count must advance once per optimizer step). */
typedef struct gml_adam_job { float* p; const float* g; float* m; float* v; int64_t n; } gml_adam_job;
#define GML_ADAM_MAX_JOBS 64
int gml_adam_many(const gml_adam_job* jobs /* host array */, int32_t njobs, float* step, uint32_t* done, float lr, float beta1,
                  float beta2, float eps, gml_stream_t stream);
/* number of partial rows gml_edge_mlp_bwd leaves for this call shape (it depends on the kernel family the call takes) */
int64_t gml_edge_mlp_bwd_parts(int64_t num_edges, int32_t S, int32_t Sout, int32_t has_split, int32_t want_gin);

int gml_version(void);
/* static string for any return code of this library (hipGetErrorString for >0) */
const char* gml_error_string(int code);

/* ---------------------------------------------------------------- CSR build (integer-exact)
 * Stable sort of the COO edge list by `key` (key = dst for the forward view, key = src for the
 * transposed view): rowptr[N+1], other[E] = the non-key endpoint of each sorted edge, perm[E] =
 * input edge id of each sorted edge (ascending inside a row).  ws: gml_csr_workspace_bytes().
 * Node ids outside [0, num_nodes) are clamped (no out-of-bounds access) and reported: the LAST int32 of the workspace
 * (byte offset gml_csr_workspace_bytes() - 4) is OR-ed with 1.  The caller zeroes that word before the call(s) that share
 * the workspace and raises when it reads non-zero (the reference's scatter raises an index error for such input). */
size_t gml_csr_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int gml_csr_from_coo(const int64_t* key, const int64_t* other_in, int64_t num_nodes, int64_t num_edges,
                     int32_t* rowptr, int32_t* other, int32_t* perm,
                     void* ws, size_t ws_bytes, gml_stream_t stream);
/* The same for keys that are ALREADY non-decreasing (edge_index2 as the reference's transform emits it is sorted by
 * source, libs/utils.py:608-609): no sort -- rowptr from the run boundaries, perm = identity, one pass.  If a key is
 * smaller than its predecessor, bit 1 (value 2) of the workspace's flag word is set and the outputs are unspecified: the
 * caller must then use gml_csr_from_coo for this view.  If two edges of the same row have decreasing other ids, bit 3
 * (value 8) is set: the view is valid, but its columns are not ascending inside every row (gml_edge_sym_flags needs them so). */
int gml_csr_from_sorted_coo(const int64_t* key, const int64_t* other_in, int64_t num_nodes, int64_t num_edges,
                            int32_t* rowptr, int32_t* other, int32_t* perm,
                            void* ws, size_t ws_bytes, gml_stream_t stream);
/* pos_t[j] = inverse(perm_fwd)[perm_t[j]]: where, in forward (target-sorted) order, the j-th
 * source-sorted edge keeps its values.  inv_scratch: E int32. */
int gml_csr_link_transpose(const int32_t* perm_fwd, const int32_t* perm_t, int64_t num_edges,
                           int32_t* inv_scratch, int32_t* pos_t, gml_stream_t stream);
/* Group records: the staging schedule of the fused kernels (gml_spectconv_fwd: group_rows = 64;
 * gml_spectconv_bwd: gml_spectconv_bwd_group_rows()).  One record of gml_csr_group_record_ints(group_rows) int32
 * per group of `group_rows` (64 or 128) consecutive rows, ceil(num_rows / group_rows) records:
 *   {first edge, #edges, smallest column id, column-window width},
 *   128-row groups: then 128 bytes, the local row each lane position of the backward kernel works on -- rows ranked
 *   by degree so that the 16 rows of a tile run near-equal edge loops, rank blocks dealt to the waves so the SIMDs
 *   stay balanced (which lane serves a row never changes the row's result).
 * Callers size LDS with the maxima of ints 1 and 3 over the records.  gml_csr_group_record_ints = int32 per record. */
int32_t gml_csr_group_record_ints(int32_t group_rows);
int gml_csr_group_info(const int32_t* rowptr, const int32_t* col, int64_t num_rows, int32_t group_rows,
                       int32_t* ginfo, gml_stream_t stream);
/* the same for two CSR views over the same rows (target- and source-keyed) in ONE launch */
int gml_csr_group_info2(const int32_t* rowptr_a, const int32_t* col_a, int32_t* ginfo_a, const int32_t* rowptr_b,
                        const int32_t* col_b, int32_t* ginfo_b, int64_t num_rows, int32_t group_rows, gml_stream_t stream);
/* One launch: a padded static-shape batch (the graphs `ids`, in that order) and its whole index structure from a device-resident data
 * set whose per-graph structure was computed once.  The reference collates every batch on the host (DataLoader, Zinc12k.py:20-22,359);
 * here a batch is gathers + offsets, because a batch is the block-diagonal union of graphs whose own structure never changes.
 * Data set side (per graph g its nodes node_ptr[g]..node_ptr[g+1] and support edges edge_ptr2[g]..edge_ptr2[g+1], graph-LOCAL node ids,
 * sorted by source inside a graph): tperm[e] = source-order position (inside its graph) of the graph's k-th TARGET-sorted edge (stable),
 * tinv its inverse, rp_src / rp_dst [node] = number of the graph's edges whose source / target is a smaller node (local row pointers),
 * es = gml_edge_presplit(edge_attr2) or NULL.  ids entries outside [0, G) = no graph.  Outputs: x_out [n_pad, F], ea_out [e2_pad, S],
 * es_out [e2_pad, 8], y_out [B + 1], valid_out [B], ptr_out [B + 2], batch_out [n_pad] (padding nodes: graph B), and the CSR arrays of
 * both views exactly as gml_csr_from_coo / _from_sorted_coo / _link_transpose give them for the assembled batch (perm == tpos;
 * perm_t is the identity).  Padding: zero-feature nodes forming graph B; zero-valued self loops dealt dmax per padding node. */
typedef struct gml_batch_desc {
    const int64_t* node_ptr; const int64_t* edge_ptr2; const float* x; const int64_t* edge_index2; const float* edge_attr2;
    const int32_t* es; const int32_t* tperm; const int32_t* tinv; const int32_t* rp_src; const int32_t* rp_dst; const float* y;
    int64_t G, E2all; int32_t F, S;
    const int64_t* ids; int32_t B, n_pad, e2_pad, dmax;
    float* x_out; float* ea_out; int32_t* es_out; float* y_out; float* valid_out; int32_t* ptr_out; int32_t* batch_out;
    int32_t* rowptr; int32_t* col; int32_t* perm; int32_t* rowptr_t; int32_t* col_t; int32_t* pos_t;
    int32_t ldx_out;   /* floats between rows of x_out (0: F); columns F .. ldx_out - 1 are written as zeros (float4-addressable rows) */
    int32_t nblk_main; /* (set by the library) */
    /* optional (both or neither): the 128-row group records of the target-keyed / source-keyed view, [ceil(n_pad / 128)][gml_csr_group_record_ints(128)]
       ints each -- what gml_csr_group_info2 would compute from the assembled index arrays, written by the same launch (round 5) */
    int32_t* ginfo128; int32_t* ginfo_t128;
} gml_batch_desc;
int gml_batch_assemble(const gml_batch_desc* d, gml_stream_t stream);
/* The same batch for ANY B (gml_batch_assemble keeps B <= 4096: its per-graph prefixes live in LDS).  gml_batch_scan (one workgroup)
 * writes the per-graph node / edge / entry prefixes of the batch into ws, int64: nlo[B] elo[B] ulo[B] nnew[B + 1] enew[B + 1] unew[B + 1]
 * Bv -- the totals are nnew[B], enew[B], unew[B]; gml_batch_assemble_any runs the scan (unless `scanned`: ws already holds it for
 * these ids) and then the element launch, with the group records of both views when ginfo128 / ginfo_t128 are given.
 *   padded mode (exact = 0): gml_batch_assemble's batch (dmax = padding edges per padding node), no host read, capturable.  A batch that
 *     does not fit n_pad / e2_pad with room for its padding edges (repeated ids can exceed the data set's bounds) keeps its leading
 *     Bv graphs that do (the others become absent slots) and ORs 4 into *bad;
 *   exact mode (exact = 1): no padding graph, nodes or edges -- n_pad / e2_pad = the totals nnew[B] / enew[B] the caller read after
 *     gml_batch_scan; ptr_out [B + 1], y_out [B], valid_out optional.  Equal to the block-diagonal batch + gml_csr_from_coo /
 *     _from_sorted_coo / _link_transpose / gml_csr_group_info.
 * Optional pairing (sym_ptr [G + 1], sym_uid / sym_mir: per graph its edge-branch entries, graph-LOCAL source-order edge positions,
 * mirror -1 = none): uid_out / mir_out (capacity e2_pad) receive every graph's entries offset by its first edge in the batch, then one
 * entry per padding edge (mirror -1), and *count their number -- gml_edge_sym_flags + compaction on the assembled batch when the
 * per-graph lists are that pass's result on each graph. */
typedef struct gml_batch_any_desc {
    gml_batch_desc b;
    int32_t exact, scanned;
    const int64_t* sym_ptr; const int32_t* sym_uid; const int32_t* sym_mir;
    int32_t* uid_out; int32_t* mir_out; int32_t* count;
    int32_t* bad;
    void* ws; size_t ws_bytes;
} gml_batch_any_desc;
size_t gml_batch_any_workspace_bytes(int32_t B);
int gml_batch_scan(const gml_batch_any_desc* a, gml_stream_t stream);
int gml_batch_assemble_any(const gml_batch_any_desc* a, gml_stream_t stream);
/* The RAW adjacency (edge_index) of the same padded batch, both CSR views, in one launch (a descriptor of its own: gml_batch_desc
 * keeps its layout).  Data set side, per graph g its raw edges edge_ptr[g]..edge_ptr[g+1] of edge_index [2, Eall] (graph-LOCAL node
 * ids, any order) and, indexed like those edges (position edge_ptr[g] + k): tperm[.] = input position (inside the graph) of the
 * graph's k-th TARGET-sorted edge, sperm[.] = the same for the k-th SOURCE-sorted edge (both stable sorts), pos[.] = target-sorted
 * position of the k-th source-sorted edge, tpos[.] = source-sorted position of the k-th target-sorted edge; rp_src / rp_dst [node] =
 * number of the graph's edges whose source / target is a smaller node.  ids / B / n_pad: as the gml_batch_assemble call that built the
 * batch.  Outputs: rowptr / col / perm, rowptr_t / col_t / perm_t, pos_t and tpos exactly as gml_csr_from_coo / _link_transpose give
 * them for the padded edge_index of dataset.DeviceDataset.batch_padded(adjacency=True): e_pad edges, the real ones in batch order,
 * then unit-valued self loops on PADDING nodes only, dealt `deal` per padding node (the caller sizes n_pad / e_pad / deal so that
 * they fit: dataset.DeviceDataset.bounds).  Optional (both or neither): ginfo128 / ginfo_t128, the 128-row group records of the
 * target- / source-keyed view (gml_csr_group_info, a second launch). */
typedef struct gml_batch_edges_desc {
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* edge_index;
    const int32_t* tperm; const int32_t* sperm; const int32_t* pos; const int32_t* tpos; const int32_t* rp_src; const int32_t* rp_dst;
    int64_t G, Eall;
    const int64_t* ids; int32_t B, n_pad, e_pad, deal;
    int32_t* rowptr; int32_t* col; int32_t* perm; int32_t* rowptr_t; int32_t* col_t; int32_t* perm_t; int32_t* pos_t; int32_t* tpos_out;
    int32_t* ginfo128; int32_t* ginfo_t128;
} gml_batch_edges_desc;
int gml_batch_assemble_edges(const gml_batch_edges_desc* d, gml_stream_t stream);
/* out[k, :] = in[perm[k], :]   (rows of `width` floats) */
int gml_gather_rows(const float* in, const int32_t* perm, float* out, int64_t rows, int32_t width,
                    gml_stream_t stream);
/* out[k, :] = in[perm[k], :] and, in the same pass, its bf16 pre-split (gml_edge_presplit of out); S <= 8 */
int gml_gather_rows_presplit(const float* in, const int32_t* perm, float* out, void* out_split, int64_t rows,
                             int32_t S, gml_stream_t stream);
/* out[perm[k], :] = in[k, :] */
int gml_scatter_rows(const float* in, const int32_t* perm, float* out, int64_t rows, int32_t width,
                     gml_stream_t stream);

/* ---------------------------------------------------------------- fused multi-support layer
 *   out[r, 0:Fout] (op)= act( sum_s ( sum_{k in row r} val[pos(k), s] * x[col[k], :] ) @ W[s] + bias )
 * rowptr/col: CSR keyed by the OUTPUT row (ginfo: gml_csr_group_info of it); pos(k) = epos ? epos[k] : k
 * (epos = NULL, i.e. values stored in the order of this CSR, is the fast path); val is [E, S] (S contiguous).
 * W element (s, i, o) lives at w[s*w_ss + i*w_si + o*w_so] so the transposed weights of the
 * backward pass need no copy.  bias may be NULL.  GML_ACCUM with GML_RELU: the activation sees the accumulated value,
 * out = relu(out + sum + bias), on every kernel (the 64-row family's own support passes accumulate this way).
 * Used for: forward (CSR by target, x = X),
 * d/dX (CSR by source, x = dOut, W transposed view, epos = pos_t). */
/* group size (64 or 128) whose records the forward wants for this shape and arithmetic; 128 additionally needs
 * epos == NULL -- the caller then passes those records and GML_GROUPS128 */
int32_t gml_spectconv_fwd_group_rows(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
/* edges of one 128-row group the ring kernel of this shape keeps in LDS at once (0: not applicable).  When the largest group of the
 * batch (int 1 of its records) exceeds it: shapes of the default ring kernel gather such groups from global memory, or -- with
 * GML_FWD_CHUNKED -- run on the chunked ring kernel, which walks them in edge chunks (sr25.py: 13 entries per row); the shapes only the
 * chunked kernel serves (6 supports, 33..48 input features) always chunk (with GML_FWD_ONEWIN at 33..48 features: twice the edges per
 * chunk).  gnn_matlang_amd.functional takes the chunked road whenever a batch needs it (GML_FWD_CHUNKS=0 in the environment: the 64-row
 * family instead); its run-to-run stability is covered by tests/stress (DESIGN s4.1c). */
int32_t gml_spectconv_fwd_stage_edges(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
/* widest column window (int 3 of the 128-row group records) the kernel this shape (and these flags, e.g. GML_FWD_CHUNKED) would run on
 * serves; 0 = no bound.  A batch with a wider group must use the 64-row family (64-row records, no GML_GROUPS128) for this call:
 * the chunked ring kernel has no road for such groups and writes NaN into their rows instead of wrong numbers. */
int32_t gml_spectconv_fwd_stage_window(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
int gml_spectconv_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos,
                      const float* val, const float* x, int64_t ldx,
                      const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                      const float* bias, float* out, int64_t ldo,
                      int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                      uint32_t flags, gml_stream_t stream);

/* The two other forward forms of the reference's operator family on the ring kernel's epilogues (one launch, projection flops
 * 1x): epilogue = 1, SpectConCatConv.forward (libs/spect_conv.py:137-158): out [N, (S + self_term) Fout], support s writes column
 * block s + self_term (+ that block's bias; block 0 of a selfconn layer = x W_last is the caller's GEMM); epilogue = 2,
 * SpectConv.forward depthwise branch (libs/spect_conv.py:81-91): w is ONE [Fin, Fout] matrix (w_ss ignored), ds
 * [S + self_term, Fin] the per-feature scales (row 0 = 1 + DSweight[0]; last row: scale of the self term when self_term):
 * out = (sum_s ds_s . H_s + ds_self . x) W + bias.  ginfo128: 128-row group records.  GML_E_UNSUPPORTED outside S in {4, 8},
 * Fin, Fout <= 32, float4-addressable x rows: the caller then maps onto gml_spectconv_fwd through transformed weights. */
int gml_spectconv_fwd_epi(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const float* val,
                          const float* x, int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                          const float* bias, float* out, int64_t ldo, int64_t num_rows, int32_t S, int32_t Fin,
                          int32_t Fout, uint32_t flags, int32_t epilogue, const float* ds, int32_t self_term,
                          gml_stream_t stream);

/* ---------------------------------------------------------------- fused backward of the layer above
 * CSR keyed by SOURCE row (rowptr/col = targets, ginfo of it), val [E, S] in that order.
 *   dx[r, :]   (op)= sum_s ( sum_{e out of r} val[e, s] g[col[e], :] ) @ W[s]^T          (NULL: skip)
 *   dval[e, s]  =  < x[r, :] @ W[s], g[col[e], :] >   for e out of r, same order as val    (NULL: skip)
 *   dw[s]       =  sum_r x[r, :]^T ( sum_{e out of r} val[e, s] g[col[e], :] )           (NULL: skip)
 * g = gradient at the layer output (after the relu mask), [N, Fout].  max_group_edges / max_group_window
 * = maxima of ginfo[:, 1] / ginfo[:, 3] (the caller reads them once per batch): they size the LDS
 * staging.  gml_spectconv_bwd_workspace_bytes returns 0 when the shape has no fused backward
 * (gml_spectconv_bwd then returns GML_E_UNSUPPORTED): the caller composes gml_spectconv_fwd on the
 * transposed view + gml_spmm_fwd + gml_sddmm instead.  flags: GML_ACCUM applies to dx; GML_F32_MFMA forces the
 * f32-input MFMA kernel (default: bf16x3 split on the bf16 matrix cores where the shape allows).
 * With 128-row groups (see below) g must be float4-addressable: 16-byte aligned, ldg % 4 == 0 and
 * ldg >= roundup4(Fout) with the padding columns zero (else GML_E_BADARG). */
/* group kind of the backward kernel this shape / flags selects: 128 (bf16x3 kernel, 8 waves), 64 (f32-MFMA kernel)
 * or 0 (no fused backward).  ginfo,
 * max_group_edges and max_group_window passed to the two functions below must be those of
 * gml_csr_group_info(..., group_rows = this value). */
int gml_spectconv_bwd_group_rows(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
size_t gml_spectconv_bwd_workspace_bytes(int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                                         int32_t max_group_edges, int32_t max_group_window, uint32_t flags);
/* Host-only: edges / target-window rows of ONE group (ints 1 / 3 of its record) the kernel this shape and these flags select keeps
 * in its staging: the 8-wave kernel's register-batched bounds, 1,024 / 192 for the 64-row kernel, the ring's capacities less its
 * alignment slack (3 edges, 7 rows) with GML_DMA_RING where the ring applies.  A group beyond either is still served -- by the
 * kernel's unstaged loops, or with GML_DMA_RING by the launch taking the 8-wave kernel instead of its ring form -- with the same
 * results; what refuses a batch is the LDS plan alone (gml_spectconv_bwd_workspace_bytes = 0).  0: no fused backward for the shape,
 * or a kernel form without a staged road (the 64-row kernel at S % 4 != 0). */
int32_t gml_spectconv_bwd_stage_edges(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
int32_t gml_spectconv_bwd_stage_window(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags);
int gml_spectconv_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const float* val,
                      const float* x, int64_t ldx, const float* g, int64_t ldg, const float* w,
                      float* dx, int64_t lddx, float* dval, float* dw,
                      int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                      int32_t max_group_edges, int32_t max_group_window, uint32_t flags,
                      void* ws, size_t ws_bytes, gml_stream_t stream);

/* gml_spectconv_bwd with  dx = conv part + dz wmix : dz [num_rows, 4] (contiguous, 16-byte aligned, columns >= nmix ignored),
 * wmix [nmix <= 4, Fin].  The ML3Layer Hadamard branch (2 nout2 <= 4 columns: Zinc12k.py's 30+2 layers) hands its share of
 * dx over as its pre-activation gradients (gml_ml3_split_bwd_ex) instead of a written-then-re-read [N, Fin] array.
 * dx must be wanted and float4-addressable; GML_ACCUM is not combined with it.  gml_spectconv_bwd_mix_supported: 1 when
 * the shape has this form (the 8-wave bf16x3 kernel, S = 8, 16 < Fin <= 32), else the caller uses dx + GML_ACCUM. */
int gml_spectconv_bwd_mix_supported(int32_t S, int32_t Fin, int32_t Fout, int32_t nmix, uint32_t flags);
int gml_spectconv_bwd_mix(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const float* val,
                          const float* x, int64_t ldx, const float* g, int64_t ldg, const float* w,
                          float* dx, int64_t lddx, float* dval, float* dw, const float* dz, const float* wmix, int32_t nmix,
                          int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                          int32_t max_group_edges, int32_t max_group_window, uint32_t flags,
                          void* ws, size_t ws_bytes, gml_stream_t stream);

/* gml_spectconv_bwd_mix for a layer whose input x is itself an ML3Layer output [relu(conv) | Hadamard columns] with nothing
 * else consuming it (libs/spect_conv.py:209-212 stacked as in Zinc12k.py:338-341): dx[:, f] for f < relu_cols is written
 * multiplied by (x[:, f] > 0), i.e. dx[:, :relu_cols] IS the gradient at the conv output of the layer below.  That layer then
 * calls gml_ml3_split_bwd_ex in its pre-masked form (y = G = NULL) and passes dx itself as g to its own conv backward
 * (columns >= its Fout are ignored there).  relu_cols = 0: gml_spectconv_bwd_mix.  Same support test. */
int gml_spectconv_bwd_mix_relu(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const float* val,
                               const float* x, int64_t ldx, const float* g, int64_t ldg, const float* w,
                               float* dx, int64_t lddx, float* dval, float* dw, const float* dz, const float* wmix, int32_t nmix,
                               int32_t relu_cols, int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                               int32_t max_group_edges, int32_t max_group_window, uint32_t flags,
                               void* ws, size_t ws_bytes, gml_stream_t stream);

/* H[r, s, :] = sum_{k in row r} val[pos(k), s] * x[col[k], :]     H is [N, S, Fin] contiguous.
 * ginfo128 (optional): 128-row group records of this CSR -> the LDS-DMA ring kernel (gml_spmm3_impl.h): any S, any Fin % 4 == 0,
 * float4-addressable x rows, epos NULL, groups of up to ~2048 staged edges (larger ones gather from global memory, same
 * results); NULL or an unsupported layout: one-row-per-lane-group kernel for any shape. */
int gml_spmm_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const int32_t* epos,
                 const float* val, const float* x, int64_t ldx, float* h,
                 int64_t num_rows, int32_t S, int32_t Fin, gml_stream_t stream);
/* the same with a hint: max_group_edges = the largest edge count of a 128-row group (max of ginfo128[:, 1]; < 0 = unknown).
 * Only the kernel choice depends on it (the register-staged 8-wave kernel while every group fits its staging, else the ring
 * kernel), never the result. */
int gml_spmm_fwd_ex(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const int32_t* epos,
                    const float* val, const float* x, int64_t ldx, float* h,
                    int64_t num_rows, int32_t S, int32_t Fin, int32_t max_group_edges, gml_stream_t stream);

/* dval[pos(k), s] = < x[col[k], :], gw[r, s, :] >  for k in row r;   gw is [N, S, Fin] contiguous */
int gml_sddmm(const int32_t* rowptr, const int32_t* col, const int32_t* epos,
              const float* x, int64_t ldx, const float* gw, float* dval,
              int64_t num_rows, int32_t S, int32_t Fin, gml_stream_t stream);

/* ---------------------------------------------------------------- ML3Layer edge branch
 *   out = relu( W4 . [ relu(W1 . e) ; tanh(W2 . e) * tanh(W3 . e) ] )      per edge e in R^S
 * w1,w2,w3: [2S, S]; w4: [Sout, 4S]  (torch.nn.Linear layout, bias-free).  S = Sout <= 16.
 * If out_t != NULL the row of edge e is also written to out_t[tpos[e], :] (the same values in a second
 * edge order: the backward kernel walks the source-sorted order); on the matrix-core kernels (2 <= S <= 8) that
 * scatter uses 32-bit byte offsets: num_edges * S * 4 must stay below 2^32 - 256, else GML_E_UNSUPPORTED (the
 * caller then permutes `out` itself).
 * ea_split (optional, S <= 8): the rows of ea split once into bf16 hi[8] | lo[8] (32 bytes per edge, 16-byte aligned)
 * by gml_edge_presplit -- the raw supports are per-batch constants, so the matrix-core kernels load their first
 * operand ready-made instead of splitting it per layer and per step.  Must describe the same ea (same edge order). */
int gml_edge_presplit(const float* ea, void* ea_split, int64_t num_edges, int32_t S, gml_stream_t stream);
int gml_edge_mlp_fwd(const float* ea, const void* ea_split, const float* w1, const float* w2, const float* w3,
                     const float* w4, float* out, const int32_t* tpos, float* out_t,
                     int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);

/* The same function for MORE than 16 supports, 16 < max(S, Sout) <= 48 (csrc/gml_edge_wide.hip; SURVEY s8(d)'s sr25 sweep at 24 and
 * 48 supports; reference: libs/spect_conv.py:190-194, 205-207): one launch, exact fp32 products, weights resident in LDS, no
 * intermediate in HBM.  ea [num_edges, S], out [num_edges, Sout]; rows 16-byte aligned where S / Sout are multiples of 4.
 * GML_E_UNSUPPORTED for max(S, Sout) <= 16 (gml_edge_mlp_fwd) or > 48.  Forward only: the host recomputes through the library
 * for the backward (no reference script trains more than 12 supports). */
int gml_edge_mlp_wide_fwd(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, float* out,
                          int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
/* Its backward, per-edge part (round 6; the autograd of libs/spect_conv.py:205-207): out = the forward's result, gout = dL/dout;
 * writes go [E, Sout] = gout * (out > 0), hid [E, 2 H2R] = relu(W1 e) | tanh(W2 e) tanh(W3 e) and gz [E, 3 H2R] = the gradients at
 * the three pre-activations, H2R = gml_edge_mlp_wide_bwd_h2r(S) = 2 S rounded up to a multiple of 4 (rows 16-byte aligned).  The
 * weight gradients are the tall contractions dW_m = gz[:, m H2R : m H2R + 2 S]^T ea and dW4[:, b 2S : (b+1) 2S] = (hid[:, b H2R : b H2R
 * + 2 S]^T go)^T (gml_xty_wide); the supports' own gradient sum_m gz_m W_m.  Exact fp32 products; same shape range as the forward. */
int32_t gml_edge_mlp_wide_bwd_h2r(int32_t S);
int gml_edge_mlp_wide_bwd(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, const float* out,
                          const float* gout, float* go, float* hid, float* gz, int64_t num_edges, int32_t S, int32_t Sout,
                          gml_stream_t stream);

/* The edge branches of a STACK of ML3Layers in one pass: every layer of Zinc12k.py:338-341 / counting.py:361-366 receives the
 * same raw supports (data.edge_attr2), so L launches of gml_edge_mlp_fwd read them L times.  out[l] [num_edges, Sout] =
 * the branch of layer l (weights w1[l] .. w4[l]) applied to the rows whose split image is ea_split (gml_edge_presplit), same
 * edge order.  The five pointer arrays (nlayers entries each) live on the HOST.  GML_E_UNSUPPORTED wherever gml_edge_mlp_plan
 * answers GML_EDGE_FAM_NONE for it -- outside S = Sout in {4, 8}, 2 <= nlayers <= 4, or under GML_EDGE_VALU=1: call gml_edge_mlp_fwd
 * per layer -- same results either way. */
int gml_edge_mlp_fwd_stack(const void* ea_split, int32_t nlayers, const float* const* w1, const float* const* w2,
                           const float* const* w3, const float* const* w4, float* const* out,
                           int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
/* The edge-branch FORWARD with fp32-class products on the bf16 matrix cores ("bf16x6": every operand cut into three bf16 pieces, the
 * products down to 2^-24 kept; csrc/gml_edge_chain6_impl.h; reference: libs/spect_conv.py:205-207, fp32 throughout).  Reads the fp32
 * rows of ea itself (no pre-split image).  gml_edge_mlp_fwd6: one layer, 2 <= S = Sout <= 16, out / tpos / out_t as gml_edge_mlp_fwd.
 * gml_edge_mlp_fwd_stack6: the layers of a stack in one pass (host pointer arrays as gml_edge_mlp_fwd_stack), S = Sout in {4, 8},
 * 1 <= nlayers <= 4.  GML_E_UNSUPPORTED outside those shapes.  The default forward of the host side since round 6: the two-piece
 * chain's ~5e-7 error on the learned supports is what moved trained-state gradients beyond 1e-4 of their term sums (DESIGN s6). */
int gml_edge_mlp_fwd6(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, float* out,
                      const int32_t* tpos, float* out_t, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
int gml_edge_mlp_fwd_stack6(const float* ea, int32_t nlayers, const float* const* w1, const float* const* w2,
                            const float* const* w3, const float* const* w4, float* const* out,
                            int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
/* The edge branch over a batch's UNIQUE support rows (csrc/gml_edge_chain_sym_impl.h).  SpectralDesign's supports sample symmetric
 * matrices (libs/utils.py:546-610), so edge (i, j) and its mirror (j, i) mostly carry bitwise the same row and the branch
 * (libs/spect_conv.py:205-207) gives both the same output.  gml_edge_sym_flags: per edge of the SOURCE-keyed view (rowptr_t, col_t of
 * gml_csr_from_coo; val_s [num_edges, S] in that order; PRECONDITION: columns ascending inside every row -- the mirror is found by
 * bisection and a repeated edge by its neighbours, so a row out of order leaves records unwritten or written twice) flag = 2
 * (evaluate, and the mirror at position mirror[k] takes the same row: src < dst, rows bitwise equal), 0 (covered by its mirror) or
 * 1 (evaluate alone); mirror = -1 unless flag = 2.  The caller
 * compacts the edges with flag > 0 into uid / mir [num_unique] (int32).  gml_edge_mlp_fwd_stack6_sym: gml_edge_mlp_fwd_stack6 over
 * those entries, out[l][uid[u]] and out[l][mir[u]] written (every row of out is written exactly once when uid / mir come from the flags).
 * gml_edge_mlp_bwd_sym: gml_edge_mlp_bwd (no gin) with gout[uid[u]] + gout[mir[u]] as the entry's output gradient; partial rows in ws:
 * gml_edge_mlp_bwd_sym_parts(num_unique, S) (ws sized by gml_edge_mlp_bwd_workspace_bytes(num_edges, ..) is large enough); dw1 .. dw4
 * all NULL leaves the partials for gml_fold_many.  2 <= S = Sout <= 16 (layer stacks: S in {4, 8}; S > 8: ea_split = the 64-byte rows of gml_edge_presplit); GML_E_UNSUPPORTED otherwise.  Exact: no tolerance --
 * rows that differ in one bit are evaluated separately. */
int gml_edge_sym_flags(const int32_t* rowptr_t, const int32_t* col_t, const float* val_s, int64_t num_rows, int64_t num_edges,
                       int32_t S, int32_t* flag, int32_t* mirror, gml_stream_t stream);
int gml_edge_mlp_fwd_stack6_sym(const float* ea, const int32_t* uid, const int32_t* mir, int64_t num_unique, int32_t nlayers,
                                const float* const* w1, const float* const* w2, const float* const* w3, const float* const* w4,
                                float* const* out, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
/* _dev: the same with the entry count on the device -- uid / mir hold `capacity` slots, *count (int32, device) of them are entries (read
 * by the kernels, clamped to [0, capacity]; a list assembled on the device, gml_batch_assemble_any, whose length the host never reads).
 * The grids are sized from capacity; the backward writes all gml_edge_mlp_bwd_sym_parts(capacity, S) partial rows (zeros where a
 * workgroup has no entry). */
int gml_edge_mlp_fwd_stack6_sym_dev(const float* ea, const int32_t* uid, const int32_t* mir, const int32_t* count, int64_t capacity,
                                    int32_t nlayers, const float* const* w1, const float* const* w2, const float* const* w3,
                                    const float* const* w4, float* const* out, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
int64_t gml_edge_mlp_bwd_sym_parts(int64_t num_unique, int32_t S);
int gml_edge_mlp_bwd_sym(const void* ea_split, const int32_t* uid, const int32_t* mir, int64_t num_unique, const float* w1,
                         const float* w2, const float* w3, const float* w4, const float* gout, float* dw1, float* dw2, float* dw3,
                         float* dw4, int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes, gml_stream_t stream);
int gml_edge_mlp_bwd_sym_dev(const void* ea_split, const int32_t* uid, const int32_t* mir, const int32_t* count, int64_t capacity,
                             const float* w1, const float* w2, const float* w3, const float* w4, const float* gout, float* dw1, float* dw2,
                             float* dw3, float* dw4, int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes,
                             gml_stream_t stream);
size_t gml_edge_mlp_bwd_workspace_bytes(int64_t num_edges, int32_t S, int32_t Sout);
/* gout: dL/dout [E, Sout].  Writes dw1..dw4 (same shapes as the weights) and, if gin != NULL,
 * dL/dea [E, S].  Intermediates are recomputed from ea. */
int gml_edge_mlp_bwd(const float* ea, const void* ea_split, const float* w1, const float* w2, const float* w3,
                     const float* w4, const float* gout, float* gin, float* dw1, float* dw2, float* dw3, float* dw4,
                     int64_t num_edges, int32_t S, int32_t Sout,
                     void* ws, size_t ws_bytes, gml_stream_t stream);
/* the edge branch on the exact-arithmetic family whatever the shape -- one edge per lane, fp32 FMAs, f32-input MFMA for the weight
 * gradients, the library's tanh: what GML_F32_MFMA is to gml_spectconv_fwd / _bwd (the default entries above take the bf16-split
 * matrix-core chains for 2 <= S <= 16).  Same arguments minus the pre-split image; the backward's dw1 .. dw4 are required. */
int gml_edge_mlp_fwd_exact(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, float* out,
                           const int32_t* tpos, float* out_t, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream);
int gml_edge_mlp_bwd_exact(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4,
                           const float* gout, float* gin, float* dw1, float* dw2, float* dw3, float* dw4,
                           int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes, gml_stream_t stream);

/* Which kernel family serves an edge-branch call (csrc/gml_edge_plan.h: the one place that decides it; answered on the host, no
 * device needed).  direction: GML_EDGE_FWD or GML_EDGE_BWD.  nlayers (forward): 0 = the single-layer entry points (gml_edge_mlp_fwd,
 * _fwd6, _fwd_exact), 1 .. 4 = the stacked ones (_fwd_stack, _fwd_stack6, _fwd_stack6_sym); ignored for the backward.  flags: one
 * arithmetic (GML_EDGE_TWO_PIECE: gml_edge_mlp_fwd / _fwd_stack / _bwd; GML_EDGE_THREE_PIECE: the ..6 forwards -- the backward
 * is two-piece either way; GML_EDGE_EXACT: the _exact entries) ored with GML_EDGE_HAS_SPLIT (ea_split is given), GML_EDGE_WANT_GIN
 * (backward: gin != NULL), GML_EDGE_DUAL (forward: out_t != NULL) and GML_EDGE_UNIQUE (the _sym entries).  Returns the family, or
 * GML_EDGE_FAM_NONE where the entry point answers GML_E_UNSUPPORTED (S != Sout, S > 16, a stack the library has no kernel for, ...)
 * and for a flag that does not belong to the direction or is not listed here.
 * GML_EDGE_VALU=1 in the environment (read once per process) turns every two-piece chain answer into GML_EDGE_FAM_VALU. */
enum { GML_EDGE_FWD = 0, GML_EDGE_BWD = 1 };
enum { GML_EDGE_TWO_PIECE = 0, GML_EDGE_THREE_PIECE = 1, GML_EDGE_EXACT = 2, GML_EDGE_ARITH_MASK = 3,
       GML_EDGE_HAS_SPLIT = 4, GML_EDGE_WANT_GIN = 8, GML_EDGE_DUAL = 16, GML_EDGE_UNIQUE = 32 };
enum { GML_EDGE_FAM_NONE = 0,
       GML_EDGE_FAM_VALU = 1,        /* one edge per lane, fp32 FMAs (csrc/gml_edge_mlp_impl.h): S = 1, exact, gin at S > 8 */
       GML_EDGE_FAM_CHAIN = 2,         /* two-piece matrix-core chain, 2 <= S <= 8 (gml_edge_chain_impl.h); stacks: S in {4, 8}, 2 .. 4 layers */
       GML_EDGE_FAM_CHAIN16 = 3,       /* two-piece, 8 < S <= 16 (gml_edge_chain16_impl.h): needs ea_split, no gin */
       GML_EDGE_FAM_CHAIN6 = 4,        /* three-piece forward, 2 <= S <= 8 (gml_edge_chain6_impl.h); stacks: S in {4, 8}, 1 .. 4 layers */
       GML_EDGE_FAM_CHAIN16X6 = 5,     /* three-piece forward, 8 < S <= 16 (gml_edge_chain16x6_impl.h) */
       GML_EDGE_FAM_SYM6 = 6,          /* unique rows, three-piece forward, 2 <= S <= 8 (gml_edge_chain_sym_impl.h) */
       GML_EDGE_FAM_SYM16X6 = 7,       /* unique rows, three-piece forward, 8 < S <= 16, one layer */
       GML_EDGE_FAM_SYM_CHAIN = 8,     /* unique rows, two-piece backward, 2 <= S <= 8 */
       GML_EDGE_FAM_SYM_CHAIN16 = 9 }; /* unique rows, two-piece backward, 8 < S <= 16 */
int32_t gml_edge_mlp_plan(int32_t direction, int32_t S, int32_t Sout, int32_t nlayers, uint32_t flags);

/* ---------------------------------------------------------------- ML3Layer forward without the edge branch
 * (libs/spect_conv.py:204-212): out[:, :nout1] = act(SpectConv(x)), out[:, nout1:nout1+F2] = tanh(fc11 x) * tanh(fc12 x).
 * Same arguments as gml_spectconv_fwd + the Hadamard weights; one launch on the 8-wave kernel when GML_GROUPS128 applies
 * and F2 <= 8, else gml_spectconv_fwd followed by gml_node_mix_fwd.  F2 = 0: conv only.
 * epos != NULL: the value row of CSR position k is val[epos[k]] -- with epos = the target-to-source position map the
 * layer consumes the edge branch's output in SOURCE order (the order the backward walks), so the edge branch writes its
 * output once instead of once per order. */
int gml_ml3_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos, const float* val,
                const float* x, int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                const float* bias, const float* w11, const float* b11, const float* w12, const float* b12,
                float* out, int64_t ldo, int64_t num_rows, int32_t S, int32_t Fin, int32_t nout1, int32_t F2,
                uint32_t flags, gml_stream_t stream);

/* ---------------------------------------------------------------- ML3Layer Hadamard branch
 *   out[r, 0:F2] = tanh(x[r] . w11^T + b11) * tanh(x[r] . w12^T + b12)      w1x: [F2, Fin] */
int gml_node_mix_fwd(const float* x, int64_t ldx, const float* w11, const float* b11,
                     const float* w12, const float* b12, float* out, int64_t ldo,
                     int64_t num_rows, int32_t Fin, int32_t F2, gml_stream_t stream);
/* Backward, one launch + fold: with z11 = x w11^T + b11, z12 likewise (recomputed from x),
 *   dx[r, :] += dL/dz11[r] . w11 + dL/dz12[r] . w12        (accumulates; dx may be NULL)
 *   dw11 = dL/dz11^T x, db11 = colsum(dL/dz11), dw12, db12 likewise.
 * gout: dL/dout with leading dimension ldg.  workspace_bytes == 0: shape not supported (caller uses GEMMs). */
size_t gml_node_mix_bwd_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t F2);
int gml_node_mix_bwd(const float* x, int64_t ldx, const float* w11, const float* b11,
                     const float* w12, const float* b12, const float* gout, int64_t ldg,
                     float* dx, int64_t lddx, float* dw11, float* db11, float* dw12, float* db12,
                     int64_t num_rows, int32_t Fin, int32_t F2, void* ws, size_t ws_bytes, gml_stream_t stream);

/* ---------------------------------------------------------------- ML3Layer output stage, backward in one pass
 * (autograd of libs/spect_conv.py:209-212: the relu on the conv part, the concat, the Hadamard branch, conv1.bias)
 *   G[:, :nout1] = gy[:, :nout1] * (y[:, :nout1] > 0), G[:, nout1:ldg] = 0      gradient at the conv output
 *   dcb          = column sums of G                                             (NULL: not wanted)
 *   dx           = dz11 w11 + dz12 w12  -- WRITTEN (follow with gml_spectconv_bwd + GML_ACCUM); NULL: not wanted
 *                  (dx is [num_rows, Fin] in rows of lddx: columns [Fin, lddx) are never written)
 *   dw11, db11, dw12, db12 as gml_node_mix_bwd, from gy[:, nout1:nout1+F2].
 * F2 == 0: no Hadamard branch (x, w*, dw*, dx ignored) -- relu mask + bias sums of a plain SpectConv.
 * workspace_bytes == 0: shape not supported (caller uses gml_relu_bwd + gml_node_mix_bwd). */
size_t gml_ml3_split_bwd_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t nout1, int32_t F2);
int gml_ml3_split_bwd(const float* gy, int64_t ldgy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                      const float* w11, const float* b11, const float* w12, const float* b12,
                      float* G, int64_t ldg, float* dx, int64_t lddx, float* dcb,
                      float* dw11, float* db11, float* dw12, float* db12,
                      int64_t num_rows, int32_t Fin, int32_t nout1, int32_t F2,
                      void* ws, size_t ws_bytes, gml_stream_t stream);

/* general form.  dz != NULL (then dx == NULL; 2 F2 <= 4): dz [num_rows, 4] = (dz11 | dz12) is written instead of dx (columns
 * beyond 2 F2 zero): the operand of gml_spectconv_bwd_mix.  gy_seg != NULL: gy holds one row per SEGMENT and row r reads
 * gy[gy_seg[r]] -- the gradient of a global add pool that directly follows the layer (Zinc12k.py:343), never expanded.
 * y == NULL and G == NULL (pre-masked form; gy_seg NULL): gy[:, :nout1] already carries the relu mask
 * (gml_spectconv_bwd_mix_relu wrote it): the saved output is not read and no G is written -- gy is G. */
int gml_ml3_split_bwd_ex(const float* gy, int64_t ldgy, const int32_t* gy_seg, const float* y, int64_t ldy,
                         const float* x, int64_t ldx, const float* w11, const float* b11, const float* w12, const float* b12,
                         float* G, int64_t ldg, float* dx, int64_t lddx, float* dz, float* dcb,
                         float* dw11, float* db11, float* dw12, float* db12,
                         int64_t num_rows, int32_t Fin, int32_t nout1, int32_t F2,
                         void* ws, size_t ws_bytes, gml_stream_t stream);

/* ---------------------------------------------------------------- glue
 * g[r, c] = (y[r, c] > 0) ? gy[r, c] : 0   for c < F, and 0 for F <= c < ldg (relu backward on a strided
 * slice; the zero padding lets consumers read aligned float4 groups) */
int gml_relu_bwd(const float* gy, int64_t ldgy, const float* y, int64_t ldy, float* g, int64_t ldg,
                 int64_t num_rows, int32_t F, gml_stream_t stream);
/* out[g, :] = sum_{r in [ptr[g], ptr[g+1])} x[r, :]  (global_add_pool over a sorted batch vector;
 * mean bit 0 divides by the segment length: global_mean_pool; bit 1 = GML_POOL_SKIP_LAST: the last segment is the padding graph of a
 * static-shape batch (gml_batch_assemble) -- its output row is written as zeros without reading its rows) */
#define GML_POOL_SKIP_LAST 2
int gml_segment_sum(const float* x, int64_t ldx, const int32_t* ptr, float* out, int64_t ldo,
                    int64_t num_segments, int32_t F, int32_t mean, gml_stream_t stream);
/* its gradient: out[r, :] = g[seg(r), :] (/ segment length when mean != 0) for r in [ptr[seg], ptr[seg+1]) */
int gml_segment_bcast(const float* g, int64_t ldg, const int32_t* ptr, float* out, int64_t ldo,
                      int64_t num_segments, int32_t F, int32_t mean, gml_stream_t stream);

/* gml_segment_sum for 32-column rows that also leaves the relu pattern of every row -- bit c of mask[row] = (x[row][c] > 0) -- and
 * the pool gradient broadcast that applies it: out[row][c] = g[seg[row]][c] * (c >= nrelu || bit c of mask[row]).  For the ML3Layer
 * directly in front of global_add_pool / global_mean_pool (Zinc12k.py:338-343, out = [relu(conv) | Hadamard columns]): its backward
 * reads 4 bytes per row instead of the saved output, and the pre-masked [num_rows, 32] gradient is what gml_spectconv_bwd_had takes.
 * F must be 32 (GML_E_UNSUPPORTED otherwise); mean: the flag word of gml_segment_sum; for a mean pool the caller divides g by the
 * segment sizes first.  Same sums, in the same order, as gml_segment_sum. */
int gml_segment_sum_mask(const float* x, int64_t ldx, const int32_t* ptr, float* out, int64_t ldo, uint32_t* mask,
                         int64_t num_segments, int32_t F, int32_t mean, gml_stream_t stream);
int gml_segment_bcast_mask(const float* g, int64_t ldg, const int32_t* seg, const uint32_t* mask, float* out, int64_t ldo,
                           int64_t num_rows, int32_t F, int32_t nrelu, gml_stream_t stream);
/* out[g, c] = max_{r in [ptr[g], ptr[g+1])} x[r, c]  (global_max_pool, /root/reference/enzymes.py:384); argmax[g, c]
 * (int32 [num_segments, F], may be NULL) = the first row that attains it; an empty segment gives 0 / -1 */
int gml_segment_max(const float* x, int64_t ldx, const int32_t* ptr, float* out, int64_t ldo, int32_t* argmax,
                    int64_t num_segments, int32_t F, gml_stream_t stream);
/* its gradient: out[r, c] = (r == argmax[seg(r), c]) ? g[seg(r), c] : 0 -- every row of every segment is written */
int gml_segment_max_bwd(const float* g, int64_t ldg, const int32_t* ptr, const int32_t* argmax, float* out, int64_t ldo,
                        int64_t num_segments, int32_t F, gml_stream_t stream);

/* ---------------------------------------------------------------- dropout (csrc/gml_dropout.hip)
 * F.dropout(x, p, training=True) in front of every layer of the TU scripts (ptc.py:349-358, enzymes.py:372-381, proteins.py:282-285)
 * and mnist75.py:299-317, with a mask that is a pure function of (seed, counter, site, e) for the logical element e = r C + c of an
 * [N, C] input -- independent of launch geometry, strides and device:
 *   Philox4x32-10 (Salmon et al., SC'11), key = (seed lo, seed hi), counter block = (j lo, j hi, site, counter lo) with j = e >> 2;
 *   u = word (e & 3) of the output;  keep e  <=>  u >= t,  t = floor(p 2^32) (host, float64; 2^32 for p = 1: nothing kept).
 * state: DEVICE pointer to int64 {seed, counter}, read by the kernel -- no host value per call, so the launch is capturable and a
 * replay uses whatever counter the device holds then.  site: which dropout of the model (the layer index).
 *   y[r, c] = keep ? x[r, c] * scale : +0.0     scale = float(1 / (1 - p)) rounded once; ONE fp32 multiply.
 * A dropped element is written as +0.0 -- not x * 0 --, so a NaN / Inf input or a negative input gives +0.0 there, never NaN or -0.0.
 * mask: packed keep bits, bit (e & 31) of word e >> 5, ceil(N C / 32) words (the unused high bits of the last word are 0).
 * One lane per 4 consecutive elements (one Philox call); float4 loads / stores when C % 4 == 0 and ldx, ldy % 4 == 0 with 16-byte
 * aligned bases, a scalar path otherwise.  N = 0 or C = 0: nothing to do, GML_OK.  t > 2^32, ld < C, NULL or misaligned pointers
 * (float / uint32 4 bytes, state 8 bytes): GML_E_BADARG.
 * gml_dropout_bwd: dx[r, c] = keep ? g[r, c] * scale : +0.0 from the saved mask; same geometry, does not touch the RNG state. */
int gml_dropout_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, uint32_t* mask, int64_t num_rows, int32_t C,
                    uint64_t t, float scale, const int64_t* state, uint32_t site, gml_stream_t stream);
int gml_dropout_bwd(const float* g, int64_t ldg, const uint32_t* mask, float* dx, int64_t lddx, int64_t num_rows, int32_t C,
                    float scale, gml_stream_t stream);

/* ---------------------------------------------------------------- pair distinguishability (csrc/gml_pairs.hip)
 * The isomorphism tests of sr25.py:281-300, graph8c.py:282-302 and exp_iso.py:284-304: which pairs of graph embeddings E [G, D] (rows
 * of ldE >= D floats, 1 <= D <= 128, G <= 65536) an untrained model never separates over many seeds.  A pair (i, j) is SEPARATED when
 *   d = sum_k |E[i, k] - E[j, k]|  >  tol            (float32 throughout; tol is the caller's float32(tol): numpy 2 casts 0.001 so)
 * with d summed in numpy's float32 sum(axis=-1) order: D < 8 sequential from 0; 8 <= D: eight accumulators over the full 8-blocks,
 * ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order.  NaN compares false and never separates.
 * Bitmap (uint64 words, zeroed by the caller once; the kernels only OR bits in, so updates accumulate over seeds):
 *   all pairs : G rows of W = ceil(G / 64) words; bit (j & 63) of word [i W + (j >> 6)] = pair (i, j), used for i < j < G only --
 *               every other bit stays 0.  G W words: 0.54 GB at G = 65536.
 *   pair list : bit (p & 63) of word [p >> 6] = pair p of pairs [P, 2] (int32); ceil(P / 64) words.  A pair with an index outside
 *               [0, G) is not read and never separates.
 * gml_pair_bitmap_words(G, P): words of the bitmap (P < 0: all pairs of G); -1 for G outside [0, 65536].
 * gml_pair_count_similar: *count (int64, device) = the number of CLEAR valid bits (pairs never separated); pairs == NULL: all pairs
 *   of G, else a list of P pairs (pairs is not read).  A memset then one accumulate launch: capturable, no host read.
 * gml_pair_list_similar: the never-separated pairs as int64 (i, j) into out [cap, 2] in bitmap order -- ascending (i, j) for all
 *   pairs, list order for a list -- by a scan (count, one-workgroup prefix, emit), so the order is the same on every run;
 *   *count = the true total even when it exceeds cap.  ws: gml_pair_list_workspace_bytes(G, P) bytes (P < 0: all pairs).
 * Arguments outside these ranges or misaligned: GML_E_BADARG. */
int64_t gml_pair_bitmap_words(int64_t G, int64_t P);
int gml_pair_distinct_all(const float* E, int64_t ldE, int64_t G, int32_t D, float tol, uint64_t* bits, gml_stream_t stream);
int gml_pair_distinct_list(const float* E, int64_t ldE, int64_t G, const int32_t* pairs, int64_t P, int32_t D, float tol,
                           uint64_t* bits, gml_stream_t stream);
int gml_pair_count_similar(const uint64_t* bits, int64_t G, const int32_t* pairs, int64_t P, int64_t* count, gml_stream_t stream);
size_t gml_pair_list_workspace_bytes(int64_t G, int64_t P);
int gml_pair_list_similar(const uint64_t* bits, int64_t G, const int32_t* pairs, int64_t P, int64_t* out, int64_t cap,
                          int64_t* count, void* ws, size_t ws_bytes, gml_stream_t stream);

/* ---------------------------------------------------------------- dense-block SpectConv (equal-size graphs, near-dense masks)
 * The TF formulation of the layer, /root/reference/libs/layers_tf.py:231-236 (s0 = matmul(support[:, i], x); out += s0 . W_i),
 * for batches of B graphs of exactly n <= 96 nodes (MNIST-75: n = 75, S = 6).
 *   gml_dense_pack       : fp32 blocks [nblocks][n][n] (row-major; transpose != 0 takes block^T) -> bf16 (hi, lo) images
 *                          img [nblocks][2][n][KP] (uint16; block = hi + lo to 2^-17 relative; KP = 32 ceil(n / 32), columns
 *                          >= n zero).  Done once per data set: the supports are constants.
 *   gml_dense_support_mm : out[(b n + r) ldo + s so + f]  =  sum_k D[b][s][r][k] . act[(b n + k) lda + s sa + f]   (f < F <= 128),
 *                          summed over s into out[(b n + r) ldo + f] when sum_s != 0.  Forward: D = the packed supports,
 *                          act = X (sa = 0), out = Hcat [B n, S Fin] (so = Fin); backward: D = the packed transposes,
 *                          act = d Hcat (sa = Fin), sum_s = 1 -> d X.  bf16x3 products, fp32 accumulate.
 *
 * The contract of the family (these two and the chained entry points gml_dense_pack_w .. gml_dense_conv_bwd_w further down;
 * tests/test_gpu_dense_abi.py holds every line of it):
 *   Shapes.   1 <= n <= 96; KP any multiple of 32 with n <= KP <= 96 (columns n .. KP - 1 of an image are zero and inert: every KP
 *             gives the same bits); 1 <= F, Fin <= 128; 1 <= Fout <= 128, except gml_dense_conv_bwd_w, which takes 1 <= Fout <= 16320
 *             (64 output columns per workgroup, at most 255 of them along Fout); S >= 1; B, nblocks >= 0.  B = 0 / nblocks = 0 is GML_OK and touches nothing
 *             (gml_dense_conv_bwd_w with B = 0 zero-fills dw and needs no workspace).
 *   Read.     Of act / x / g exactly rows [0, B n) and the columns the formula names (s sa + f, f < F): padding columns and rows
 *             behind row B n - 1 are never read, NaN there reaches nothing.  Images and weight images: exactly their size.
 *   Written.  Exactly rows [0, B n) x the columns the formula names; columns between the supports' slices (so > F), padding
 *             columns up to ldo and everything behind row B n - 1 keep their bytes.  gml_dense_pack writes exactly
 *             nblocks * 2 * n * KP uint16; gml_dense_pack_w / _wt exactly gml_dense_wimg_elems / gml_dense_wimgt_elems int16.
 *   Alignment. Images, weight images and workspaces: 16 bytes.  act / x / g / out / out2 / hcat / dx: 4 bytes; an operand whose
 *             width, leading dimension and column stride (sa, so) are multiples of 4 floats and which starts on a 16-byte boundary
 *             moves as float4, any other element by element -- same bits either way (gml_dense_plan answers which).
 *   Errors, in this order, nothing written: GML_E_BADARG for a NULL required pointer (bias, hcat and dw may be NULL), a negative
 *             sa / so, or a leading dimension below the columns the formula names (gml_dense_support_mm: (S - 1) sa + F of act,
 *             (S - 1) so + F of out, F when sum_s; the others: Fin / Fout); GML_E_UNSUPPORTED outside the shapes above; GML_E_WORKSPACE (gml_dense_conv_bwd_w,
 *             B > 0) for a NULL or short workspace.
 *   Determinism. No atomics: two launches on the same inputs agree bit for bit. */
int gml_dense_pack(const float* blocks, uint16_t* img, int64_t nblocks, int32_t n, int32_t KP, int32_t transpose,
                   gml_stream_t stream);
int gml_dense_support_mm(const uint16_t* dimg, const float* act, int64_t lda, int32_t sa, float* out, int64_t ldo,
                         int32_t so, int32_t sum_s, int32_t B, int32_t S, int32_t n, int32_t KP, int32_t F,
                         gml_stream_t stream);
/* Which kernel template and which roads a call of the family takes (csrc/gml_dense.hip: the one place that decides them; the entry
 * points launch what this answers; answered on the host, no launch, pointers are not dereferenced).  Arguments as the entry point
 * names them: SUPPORT_MM (in = act, ld_in = lda, s_in = sa, out, ld_out = ldo, s_out = so, F); CONV_FWD (in = x, ld_in = ldx,
 * out = hcat or NULL, out2, ld_out2 = ldo2, F = Fin, Fout); CONV_BWD_X (out = dx, ld_out = lddx, F = Fin, Fout); CONV_BWD_W
 * (in = x, ld_in = ldx, F = Fin, Fout); the others are ignored.  Returns the GML_DENSE_VEC_* bits of the operands that move as
 * float4, | NFT << 8 (feature tiles of the template: 1, 2, 4, 8) | NOT << 16 (output tiles: 4 up to Fout = 64, else 8; CONV_BWD_W:
 * its workgroups along Fout, at most 255; SUPPORT_MM: 0); GML_E_BADARG for an unknown entry, GML_E_UNSUPPORTED outside the widths
 * above (CONV_BWD_W: Fout > 16320). */
enum { GML_DENSE_SUPPORT_MM = 0, GML_DENSE_CONV_FWD = 1, GML_DENSE_CONV_BWD_X = 2, GML_DENSE_CONV_BWD_W = 3 };
enum { GML_DENSE_VEC_IN = 1, GML_DENSE_VEC_OUT = 2 /* out / hcat / dx */, GML_DENSE_VEC_OUT2 = 4 };
int32_t gml_dense_plan(int32_t entry, const void* in, int64_t ld_in, int32_t s_in, const void* out, int64_t ld_out, int32_t s_out,
                       const void* out2, int64_t ld_out2, int32_t F, int32_t Fout);
/* The same product for ONE large graph: 96 < n <= 1024 nodes, F <= 64, any S >= 1 (the 30 x 30 grid of filtering.py: n = 900, a
 * 40 % full mask, S = 11).  Images in the format above with nblocks = S (gml_dense_big_pack; KP = 32 ceil(n / 32)).
 *   gml_dense_big_support_mm : out[r ldo + s so + f]  =  sum_k D[s][r][k] . act[k lda + s sa + f], summed over s into out[r ldo + f]
 *                              when sum_s != 0.  Rows k >= n of act are never read; only the F columns named above are written.
 * The work is cut across (support, 64-row block, K slice); with a K split or the sum over s the items write partial tiles into ws
 * (gml_dense_big_workspace_bytes(S, n, F, sum_s) bytes, 16-byte aligned; 0 = none needed) and a second launch adds them in
 * ascending (s, slice) order: no float atomics, bitwise the same result on every run.  bf16x3 products, fp32 accumulate.
 * GML_E_UNSUPPORTED outside 96 < n <= 1024, 1 <= F <= 64, KP = 32 ceil(n / 32); GML_E_WORKSPACE when ws is too small. */
size_t gml_dense_big_workspace_bytes(int32_t S, int32_t n, int32_t F, int32_t sum_s);
int gml_dense_big_pack(const float* blocks, uint16_t* img, int64_t nblocks, int32_t n, int32_t KP, int32_t transpose,
                       gml_stream_t stream);
int gml_dense_big_support_mm(const uint16_t* dimg, const float* act, int64_t lda, int32_t sa, float* out, int64_t ldo,
                             int32_t so, int32_t sum_s, int32_t S, int32_t n, int32_t KP, int32_t F, void* ws, size_t ws_bytes,
                             gml_stream_t stream);
/* The same product for a BATCH of equal-size graphs of 96 < n <= 256 nodes, F <= 128, any S >= 1 (freqclass.py: graphs of 200 nodes,
 * S = 6, layers 66 -> 64 + 2).  csrc/gml_dense_mid.hip.  dimg is a bank [G][S][2][n][KP] of the images above
 * (gml_dense_big_pack with nblocks = G S; KP = 32 ceil(n / 32)); graph b of the batch reads slot g_b = gid ? gid[b] : b (gid int32 [B],
 * the caller guarantees 0 <= gid[b] < G; gid = NULL needs B <= G).
 *   gml_dense_mid_support_mm : out[(b n + r) ldo + s so + f]  =  sum_{k < n} D[g_b][s][r][k] . act[(b n + k) lda + s sa + f]   (r < n, f < F),
 *                              summed over s into out[(b n + r) ldo + f] when sum_s != 0.  Forward: sa = 0, so = F; adjoint: the
 *                              transposed bank, sa = F, sum_s = 1.  Rows >= B n of act and columns outside [s sa, s sa + F) are never
 *                              read; only the named columns of rows < B n of out are written.  Rows of any stride: float4 accesses
 *                              where rows are 16-byte addressable, scalar ones otherwise.
 * One workgroup per (graph, 64-row block, support) -- per (graph, 64-row block) with sum_s, the supports in ascending order -- forms
 * the whole K sum: one launch, no workspace, no atomics, bitwise the same result on every run.  bf16x3 products, fp32 accumulate.
 * GML_E_UNSUPPORTED outside 96 < n <= 256, 1 <= F <= 128, KP = 32 ceil(n / 32), S, B, G >= 1; GML_E_BADARG for NULL dimg / act / out,
 * images that are not 16-byte aligned, or lda / ldo smaller than the columns used.  Nothing is launched on either. */
int gml_dense_mid_support_mm(const uint16_t* dimg, const int32_t* gid, const float* act, int64_t lda, int32_t sa, float* out,
                             int64_t ldo, int32_t so, int32_t sum_s, int32_t B, int32_t G, int32_t S, int32_t n, int32_t KP,
                             int32_t F, gml_stream_t stream);
/* The same product for a batch of graphs of DIFFERENT sizes, every one of at most NP = 128 nodes, with optional dropout of the
 * support entries (the TF GNNML3 of enzymes_contfeats_gnnml3_tf.py; libs/layers_tf.py:276-298).  csrc/gml_dense_rag.hip.
 *   pack       : the bank of a whole data set of G graphs from its collated COO supports (edge_index2 int64 [2][E] with global node
 *                ids, edge_attr2 fp32 [E][S], batch int64 [N] = the graph of each node, ptr int32 [G + 1]): two bf16 (hi, lo) images
 *                [G][S][2][NP][NP], img_fwd[g][s][.][j - ptr[g]][i - ptr[g]] = edge_attr2[e][s] for edge e = (i -> j) and img_bwd
 *                its transposes; hi + lo as the equal-size pack above; entries without an edge are zero (the function zero-fills both
 *                images itself).  The caller guarantees n_g <= NP: edges that fall outside their graph's block are skipped.
 *   mask       : the keep bits of ONE dropout site for a batch of B graphs (ptr int32 [B + 1]), uint32 [B][S][NP][4] each way: bit
 *                (k & 31) of word (k >> 5) of row r of mask_fwd is the decision of the logical element e = ((b S + s) NP + r) NP + k
 *                under the dropout contract above (Philox4x32-10, counter block (j lo, j hi, site, counter lo), j = e >> 2, word
 *                e & 3, keep iff draw >= t); mask_bwd (may be NULL) holds the same decisions transposed (bit (r & 31) of word (r >> 5)
 *                of row k).  Bits with r >= n_b or k >= n_b are zero.  b is the position in the batch, not the bank slot.
 *   support_mm : out[(ptr[b] + r) ldo + s so + f]  =  scale . sum_{k < n_b} keep(b, s, r, k) . D[gid[b]][s][r][k] . act[(ptr[b] + k) lda + s sa + f]
 *                for r < n_b = ptr[b + 1] - ptr[b] <= NP and f < F <= 256, summed over s into out[(ptr[b] + r) ldo + f] when sum_s != 0.
 *                gid int32 [B] maps a batch position to a bank slot (< G; NULL = the identity), the node rows are compact (no padding
 *                rows).  mask == NULL: no dropout, scale is taken as 1.  The direction is chosen by the image and the bits passed:
 *                (img_fwd, mask_fwd) with sa = 0 gives Hcat, (img_bwd, mask_bwd) with sa = Fin, sum_s = 1 its adjoint.  bf16x3
 *                products, fp32 accumulate, no atomics: two launches on the same inputs agree bitwise.
 * GML_E_UNSUPPORTED outside 1 <= F <= 256, S >= 1; GML_E_BADARG for NULL or misaligned pointers (images and bits 16 bytes, the rest
 * their element size) and for lda / ldo smaller than the columns used; nothing is launched then. */
int gml_dense_rag_pack(const int64_t* edge_index2, const float* edge_attr2, const int64_t* batch, const int32_t* ptr,
                       uint16_t* img_fwd, uint16_t* img_bwd, int64_t E, int64_t N, int32_t G, int32_t S, gml_stream_t stream);
int gml_dense_rag_mask(const int32_t* ptr, uint32_t* mask_fwd, uint32_t* mask_bwd, int32_t B, int32_t S, uint64_t t,
                       const int64_t* state, uint32_t site, gml_stream_t stream);
int gml_dense_rag_support_mm(const uint16_t* dimg, const uint32_t* mask, float scale, const int32_t* gid, const int32_t* ptr,
                             const float* act, int64_t lda, int32_t sa, float* out, int64_t ldo, int32_t so, int32_t sum_s,
                             int32_t B, int32_t S, int32_t G, int32_t F, gml_stream_t stream);

/* ---------------------------------------------------------------- node-level readout + masked squared loss (filtering.py:268, :320-327)
 *   gml_node_head_fwd : pre[r] = x[r ldx ..] . w + b[0]  (F <= 64; b may be NULL), loss[0] = sum_r (mask[r ldm] (pre[r] - y[r ldy]))^2;
 *                       stats (optional, 4 floats) = {loss, ss_res, ss_tot, count} over the rows with mask == 1: ss_res = sum (y - pre)^2,
 *                       ss_tot = sum (y - ybar)^2 with ybar the mean of y over those rows, formed first (r2 = 1 - ss_res / ss_tot).
 *   gml_node_head_bwd : g[0] = d / d loss (device scalar): dpre = g 2 mask^2 (pre - y); dx[r lddx + f] = dpre[r] w[f];
 *                       dw[f] = sum_r dpre[r] x[r][f]; db[0] = sum_r dpre[r]  (dx / dw / db may each be NULL).
 * One launch each, any N, fixed-order sums, no host read: capturable. */
int gml_node_head_fwd(const float* x, int64_t ldx, const float* w, const float* b, const float* y, int64_t ldy, const float* mask,
                      int64_t ldm, int64_t N, int32_t F, float* pre, float* loss, float* stats, gml_stream_t stream);
int gml_node_head_bwd(const float* g, const float* x, int64_t ldx, const float* w, const float* pre, const float* y, int64_t ldy,
                      const float* mask, int64_t ldm, int64_t N, int32_t F, float* dx, int64_t lddx, float* dw, float* db,
                      gml_stream_t stream);

/* The layer in ONE launch, as libs/layers_tf.py:231-236 forms it (matmul(support, x) then the projection by W_i): the support
 * product's accumulators are the projection's operand, Hcat never goes through a library GEMM.
 *   gml_dense_pack_w   : weight [S][Fin][Fout] fp32 -> bf16 (hi, lo) projection fragments (gml_dense_wimg_elems int16 elements)
 *   gml_dense_conv_fwd : out2[(b n + r) ldo2 + o] = act?( sum_s sum_f (sum_k D[b][s][r][k] x[(b n + k) ldx + f]) W[s][f][o] + bias[o] );
 *                        hcat (optional, [B n, S Fin] contiguous) receives D_s X for the caller's weight gradient, bit for bit what
 *                        gml_dense_support_mm(sum_s = 0, so = Fin) writes; out2 has the same bits with and without it.  relu != 0:
 *                        max(., 0), a deselected element is +0.0.  bias may be NULL.  Fin, Fout <= 128.  Contract: see the
 *                        dense-block paragraph above. */
size_t gml_dense_wimg_elems(int32_t S, int32_t Fin, int32_t Fout);
int gml_dense_pack_w(const float* w, uint16_t* wimg, int32_t S, int32_t Fin, int32_t Fout, void* stream);
int gml_dense_conv_fwd(const uint16_t* dimg, const float* x, int64_t ldx, const uint16_t* wimg, const float* bias,
                       float* out2, int64_t ldo2, float* hcat, int32_t B, int32_t S, int32_t n, int32_t KP, int32_t Fin,
                       int32_t Fout, int32_t relu, void* stream);
/* and its gradient w.r.t. x in one launch: dx[(b n + i) lddx + f] = sum_s sum_j D[b][s][j][i] (sum_o g[(b n + j) ldg + o] W[s][f][o])
 * -- the projection g W_s^T per row tile, then the support product on the TRANSPOSED packed blocks (gml_dense_pack(transpose = 1));
 * d Hcat is never materialised.  wimgT: gml_dense_pack_wt (gml_dense_wimgt_elems int16 elements). */
size_t gml_dense_wimgt_elems(int32_t S, int32_t Fin, int32_t Fout);
int gml_dense_pack_wt(const float* w, uint16_t* wimgT, int32_t S, int32_t Fin, int32_t Fout, void* stream);
int gml_dense_conv_bwd_x(const uint16_t* dimgT, const float* g, int64_t ldg, const uint16_t* wimgT, float* dx, int64_t lddx,
                         int32_t B, int32_t S, int32_t n, int32_t KP, int32_t Fin, int32_t Fout, void* stream);
/* the layer's weight gradient WITHOUT Hcat and without a library GEMM: dW[s][f][o] = sum_b sum_j (D[b][s] X[b])[j][f] g[b n + j][o] -- the
 * support product recomputed per graph on the matrix cores and contracted with g over the graph's rows (K = 16 MFMAs on the
 * untransposed product), per-slice partial sums in ws ([gml_dense_dw_slices(B)][S][Fin][Fout]) folded in slice order into dw
 * (dw == NULL: the partials stay for gml_fold_many).  dimg: the forward images (gml_dense_pack(transpose = 0)); Fin <= 128,
 * 1 <= Fout <= 16320 (255 workgroups of 64 columns; GML_E_UNSUPPORTED beyond).  Slices: gml_dense_dw_slices(B) = min(max(B, 1), 64); slice i owns the graphs [i per, min((i + 1) per, B)) with
 * per = ceil(B / slices) and writes its whole [S][Fin][Fout] partial -- zeros (+0.0) when it owns no graph (B = 65: slices 33 .. 63),
 * so the fold never reads an unwritten float.  ws: gml_dense_dw_workspace_bytes(B, S, Fin, Fout) = slices S Fin Fout floats, 16-byte
 * aligned, all of it written and nothing behind it; 0 for B <= 0.  NULL or short: GML_E_WORKSPACE. */
int32_t gml_dense_dw_slices(int32_t B);
size_t gml_dense_dw_workspace_bytes(int32_t B, int32_t S, int32_t Fin, int32_t Fout);
int gml_dense_conv_bwd_w(const uint16_t* dimg, const float* x, int64_t ldx, const float* g, int64_t ldg, float* dw,
                         int32_t B, int32_t S, int32_t n, int32_t KP, int32_t Fin, int32_t Fout, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- support precompute on the device (adjacent step, P1)
 * SpectralDesign.__call__ (libs/utils.py:546-610) for a batch of graphs with at most 80 nodes each (larger: host
 * implementation).  node_ptr [B+1], edge_ptr [B+1]: graph b owns nodes [node_ptr[b], node_ptr[b+1]) and the edges
 * [edge_ptr[b], edge_ptr[b+1]) of edge_index [2, e_total] (int64, global node ids).
 *   gml_spectral_count : nnz[b] = number of entries of the mask M_b (A or (A+I) squared recfield-1 times, > 0);
 *   gml_spectral_design: with out_ptr = exclusive scan of nnz ([B+1], int64) writes, at out_ptr[b], the row-major COO of
 *     M_b (edge_index2 [2, m_total] int64, global ids) and per entry the S = nfreq + 1 (+1) support values
 *     (edge_attr2 [m_total, S]: nfreq Gaussian band-pass filters of the normalised-Laplacian spectrum -- or of A's when
 *     laplacien == 0 --, the identity, and A when addadj), plus lmax[b] = largest Laplacian eigenvalue.
 * Eigenproblems in float64 (cyclic Jacobi in LDS); has_vmax/vmax = fixed upper end of the frequency grid. */
int gml_spectral_count(const int32_t* node_ptr, const int32_t* edge_ptr, const int64_t* edge_index, int64_t e_total,
                       int64_t num_graphs, int32_t max_nodes, int32_t recfield, int32_t* nnz, gml_stream_t stream);
int gml_spectral_design(const int32_t* node_ptr, const int32_t* edge_ptr, const int64_t* edge_index, int64_t e_total,
                        int64_t num_graphs, int32_t max_nodes, int32_t recfield, int32_t nfreq, double dv,
                        int32_t has_vmax, double vmax, int32_t laplacien, int32_t addadj, const int64_t* out_ptr,
                        int64_t m_total, int64_t* edge_index2, float* edge_attr2, float* lmax, gml_stream_t stream);

/* torch.nn.BatchNorm1d in training mode over the rows of x [num_rows, C] (mutag.py:272-288: one between every two layers): batch
 * statistics (mean, BIASED variance, rstd = 1 / sqrt(var + eps)), y = (x - mean) rstd weight + bias, and the backward: sum_dy = d bias,
 * sum_dyxhat = d weight, dx = (dy - sum_dy / n - xhat sum_dyxhat / n) rstd weight.  C <= 64, C % 4 == 0, float4-addressable rows; other
 * shapes: GML_E_UNSUPPORTED.  weight / bias may be NULL (affine=False).  ws: gml_bn_workspace_bytes(num_rows).
 * Alignment: x, y, dy, dx AND every per-column vector a launch READS -- mean, rstd, weight, bias, sum_dy, sum_dyxhat -- AND ws are
 * accessed as 16-byte vectors and must be 16-byte aligned (a leading dimension that is a multiple of 4 keeps every row so), else
 * GML_E_UNSUPPORTED, checked on the host before anything is launched.  The vectors a launch WRITES (mean, var, rstd of _stats, sum_dy,
 * sum_dyxhat of _bwd_sums, count) need float alignment only.  The same holds for the masked entry points below. */
size_t gml_bn_workspace_bytes(int64_t num_rows);
int gml_bn_stats(const float* x, int64_t ldx, int64_t num_rows, int32_t C, float eps, float* mean, float* var, float* rstd,
                 void* ws, size_t ws_bytes, gml_stream_t stream);
int gml_bn_apply(const float* x, int64_t ldx, int64_t num_rows, int32_t C, const float* mean, const float* rstd, const float* weight,
                 const float* bias, float* y, int64_t ldy, gml_stream_t stream);
int gml_bn_bwd_sums(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t num_rows, int32_t C, const float* mean,
                    const float* rstd, float* sum_dy, float* sum_dyxhat, void* ws, size_t ws_bytes, gml_stream_t stream);
int gml_bn_bwd_apply(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t num_rows, int32_t C, const float* mean,
                     const float* rstd, const float* weight, const float* sum_dy, const float* sum_dyxhat, float* dx, int64_t lddx,
                     gml_stream_t stream);
/* The same over a padded batch (dataset.py static shapes): ROW VALIDITY is device-resident, a per-row float vector row_valid
 * [num_rows] -- row r takes part iff row_valid[r] != 0 (padding nodes at the end of a node batch, absent graph slots anywhere in a
 * pooled one).  stats: mean / biased variance over the valid rows, their count n -> count[0] (computed on the device; n == 0: mean 0,
 * var 0).  apply: y of the valid rows, exact zeros on the others.  bwd_sums: over the valid rows.  bwd_apply: dx of the valid rows
 * with n = count[0], exact zeros on the others.  running_update: running_mean / running_var <- (1 - momentum) r + momentum stat, the
 * variance unbiased by n / (n - 1) with n read on the device; n < 2 leaves both untouched.  No host read anywhere (capturable); fixed
 * reduction order (repeat runs are bitwise equal).  Shapes as above.  ws: gml_bn_masked_workspace_bytes(num_rows). */
size_t gml_bn_masked_workspace_bytes(int64_t num_rows);
int gml_bn_masked_stats(const float* x, int64_t ldx, const float* row_valid, int64_t num_rows, int32_t C, float eps, float* mean, float* var,
                        float* rstd, float* count, void* ws, size_t ws_bytes, gml_stream_t stream);
int gml_bn_masked_apply(const float* x, int64_t ldx, const float* row_valid, int64_t num_rows, int32_t C, const float* mean, const float* rstd,
                        const float* weight, const float* bias, float* y, int64_t ldy, gml_stream_t stream);
int gml_bn_masked_bwd_sums(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* row_valid, int64_t num_rows, int32_t C,
                           const float* mean, const float* rstd, float* sum_dy, float* sum_dyxhat, void* ws, size_t ws_bytes,
                           gml_stream_t stream);
int gml_bn_masked_bwd_apply(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* row_valid, int64_t num_rows, int32_t C,
                            const float* mean, const float* rstd, const float* weight, const float* sum_dy, const float* sum_dyxhat,
                            const float* count, float* dx, int64_t lddx, gml_stream_t stream);
int gml_bn_masked_running_update(const float* count, const float* mean, const float* var, int32_t C, float momentum, float* running_mean,
                                 float* running_var, gml_stream_t stream);

/* out[i, j] = sum_r A[r, i] * B[r, j]  (a, b <= 64): weight gradient g^T x of a small dense layer over n rows
 * (readout head fc1 / fc2, Zinc12k.py:343-345), rows split over the chip, fixed summation order */
size_t gml_xty_workspace_bytes(int64_t n, int32_t a, int32_t b);
int gml_xty(const float* A, int64_t lda, const float* B, int64_t ldb, float* out, int64_t n, int32_t a, int32_t b,
            void* ws, size_t ws_bytes, gml_stream_t stream);

/* out[i, j] = sum_r A[r, i] * B[r, j] for a wide A (a <= 4096 columns) and b <= 128: the dense-block layer's weight gradient
 * dW = Hcat^T g (libs/layers_tf.py:231-236, its autograd: a = S Fin, b = Fout) on the bf16 matrix cores (bf16x3 split products, fp32
 * accumulate), rows along K through transposing LDS reads; per-row-range partials folded in order.  ws: gml_xty_wide_workspace_bytes
 * (16-byte aligned; all of it is written, nothing behind it).  Rows behind row n - 1 and columns beyond a / b are never read.
 * Answers, in this order, nothing written: GML_E_UNSUPPORTED unless n >= 0, 1 <= a <= 4096, 1 <= b <= 128 (gml_xty_wide_supported);
 * GML_E_BADARG for out == NULL, lda < a or ldb < b; n == 0 zero-fills out (A, B and ws may be NULL) and is GML_OK; GML_E_BADARG for
 * A == NULL or B == NULL; GML_E_WORKSPACE for a NULL or short ws. */
int gml_xty_wide_supported(int64_t n, int32_t a, int32_t b);
size_t gml_xty_wide_workspace_bytes(int64_t n, int32_t a, int32_t b);
int gml_xty_wide(const float* A, int64_t lda, const float* B, int64_t ldb, float* out, int64_t n, int32_t a, int32_t b,
                 void* ws, size_t ws_bytes, gml_stream_t stream);

/* Readout head + L1-sum loss of the ZINC GNNML3 in one launch each way (Zinc12k.py:343-345, :365) for the reference's regime, a
 * batch of 64 graphs, where head, loss and their backward were ~20 of the step's 70 launches (csrc/gml_head.hip):
 *   loss[0] = sum_{r < rows_loss} valid[r] |w2 . relu(W1 p[r] + b1) + b2 - y[r]|     p [rows, nin] pooled features, W1 [nh, nin]
 * rows >= rows_loss (the padding graph of a static batch) enter neither the loss nor any gradient.  `valid` is a WEIGHT, and the rows
 * >= rows_loss are left out by a zero factor: those rows of p ARE read (and their logits written to pre), so a non-finite value in
 * them is the caller's error -- unlike masked BatchNorm's invalid rows, which are never used.  This holds for all three heads
 * (gml_head_l1_*, gml_head_l1_big_*, gml_head_bce_*).  pre (optional): logits of all
 * rows.  The backward recomputes from p and scales by gscale[0] (device scalar, NULL = 1): gp [rows, nin], dw1 [nh, nin], db1 [nh]
 * (NULL allowed), dw2 [nh], db2 [1] (NULL allowed).  One workgroup: rows <= 256, nin, nh <= 64 and everything in LDS, else
 * GML_E_UNSUPPORTED (large batches run the general path: library GEMMs + gml_xty). */
int gml_head_l1_fwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                    const float* w2, const float* b2, int32_t rows, int32_t rows_loss, int32_t nin, int32_t nh,
                    float* loss, float* pre, gml_stream_t stream);
/* gml_head_l1_fwd + loss_sum[0] += loss (NULL: none): the epoch's running loss (Zinc12k.py:366) without a launch of its own */
int gml_head_l1_fwd_acc(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                        const float* w2, const float* b2, int32_t rows, int32_t rows_loss, int32_t nin, int32_t nh,
                        float* loss, float* loss_sum, float* pre, gml_stream_t stream);
int gml_head_l1_bwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                    const float* w2, const float* b2, int32_t rows, int32_t rows_loss, int32_t nin, int32_t nh,
                    const float* gscale, float* gp, int64_t ldgp, float* dw1, float* db1, float* dw2, float* db2,
                    gml_stream_t stream);

/* The same head + loss for ANY number of rows (nin = nh = 32: GNNML3's 30 + 2 features, fc1 32 -> 32; GML_E_UNSUPPORTED otherwise --
 * the caller keeps its general road): one pass forward + the fold of the per-workgroup loss partials, one pass backward (forward
 * recomputed; gp written; dw1 / db1 / dw2 / db2 contracted over the rows with exact f32 matrix-core products, one partial per
 * workgroup) + the fixed-order fold.  ws: gml_head_l1_big_workspace_floats(rows, nin, nh) floats (0: shape not served).  _bwd with
 * dw1 = dw2 = NULL: the partials [parts][1089] (dw1 | db1 | dw2 | db2) stay in ws for gml_fold_many, parts = workspace_floats / 1089.
 * Replaces ~16 launches of the general road (Zinc12k.py:343-345, :365 at the bench's batch size). */
size_t gml_head_l1_big_workspace_floats(int64_t rows, int32_t nin, int32_t nh);
int gml_head_l1_big_fwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                        const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh,
                        float* loss, float* loss_sum, void* ws, size_t ws_floats, gml_stream_t stream);
int gml_head_l1_big_bwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                        const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh,
                        const float* gscale, float* gp, int64_t ldgp, float* dw1, float* db1, float* dw2, float* db2,
                        void* ws, size_t ws_floats, gml_stream_t stream);

/* Readout head + sum binary cross-entropy ON LOGITS + number of correct predictions of the EXP classification experiment
 * (exp_classify.py:293-295 / :260-262 head, :328-329 loss, :334 accuracy; csrc/gml_head_bce.hip), one pass each way:
 *   h = act(W1 p[r] + b1), z_r = w2 . h + b2                 p [rows, nin] pooled features, W1 [nh, nin]; act: 1 = relu, 0 = identity
 *   l_r = y_r softplus(-z_r) + (1 - y_r) softplus(z_r),      softplus(t) = max(t, 0) + log1p(exp(-|t|)), each term capped at 100
 *   loss[0] = sum_{r < rows_loss} valid[r] l_r               (valid NULL: all ones; labels y are 0 or 1)
 *   ok      = sum_{r < rows_loss} valid[r] [(z_r > 0) == (y_r == 1)],   n = number of rows r < rows_loss with valid[r] != 0
 * pre (optional): the logits of all `rows` rows.  stats (optional, 3 floats) is ACCUMULATED: stats += {loss, ok, n} -- an epoch's
 * loss and accuracy (ok / n) with no launch and no host read of their own; the caller zeroes it.  The forward stands alone
 * (evaluation).  The backward recomputes from p: dz_r = gscale[0] valid[r] (sigmoid(z_r) - y_r) for r < rows_loss, else 0 (gscale:
 * device scalar, NULL = 1); gp [rows, nin] (ldgp >= nin; rows >= rows_loss -- the padding graph of a static batch -- and rows with
 * valid == 0 receive exact zeros), dw1 [nh, nin], db1 [nh] (NULL allowed), dw2 [nh], db2 [1] (NULL allowed).
 * 1 <= nin, nh <= 64, neither needs to be a multiple of 4 and no pointer needs more than float alignment; b1, b2, valid may be NULL;
 * ldp >= nin; any rows >= 1.  GML_E_UNSUPPORTED outside these widths or for another act, GML_E_BADARG for a null or short argument.
 * rows <= 256: one launch, no workspace (ws may be NULL).  Beyond: each workgroup writes one record  dw1 | db1 | dw2 | db2 | loss | ok | n
 * (nh nin + 2 nh + 4 floats) to ws and a second small launch adds the records in ascending workgroup order;
 * ws: gml_head_bce_workspace_floats(rows, nin, nh) floats (0 for rows <= 256 and for unserved shapes), else GML_E_WORKSPACE.
 * No atomics, fixed summation orders: the same input gives the same bits.  Products are plain fp32 FMAs, exp / log1p the device
 * library's.  No allocation, no sync, no host read: capturable.
 * Two departures from the reference's F.binary_cross_entropy(torch.sigmoid(z), y, reduction='sum') and torch.round(sigmoid(z)):
 *   1. for |z| above ~16.6 the reference's fp32 sigmoid rounds to 0 or 1: its loss then jumps to the clamp 100 and its gradient to 0.
 *      Here the formula above holds throughout: the true loss up to the cap, the gradient sigmoid(z) - y.  The two agree wherever the
 *      reference's own arithmetic is meaningful.
 *   2. torch.round(sigmoid(z)) calls class 1 when sigmoid(z) > 0.5, which in fp32 differs from z > 0 only for 0 < z < 2.4e-7; here z > 0. */
size_t gml_head_bce_workspace_floats(int64_t rows, int32_t nin, int32_t nh);
int gml_head_bce_fwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                     const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh, int32_t act,
                     float* loss, float* pre, float* stats, void* ws, size_t ws_floats, gml_stream_t stream);
int gml_head_bce_bwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                     const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh, int32_t act,
                     const float* gscale, float* gp, int64_t ldgp, float* dw1, float* db1, float* dw2, float* db2,
                     void* ws, size_t ws_floats, gml_stream_t stream);

/* GNNML1 block in one launch each way (csrc/gml_gnnml1.hip, inputs wider than 64 and mode 3: csrc/gml_gnnml1_wide.hip) -- /root/reference/sr25.py:231-240 (graph8c.py: the same class),
 * mnist75.py:296-318, mutag.py:253-262.  a = fc_i1(x), c = conv_i1(x) = (A^T x) Wc + bc (SpectConv, K = 1, selfconn = False,
 * libs/spect_conv.py:64-96 with one support), f2 = fc_i2(x), f3 = fc_i3(x):
 *   mode 0: out [N, n] = act(a + c + f2 * f3)   (n1 = n2 = n3 = n)        mode 1: out [N, n1 + n2 + n3] = [act(a) | act(c) | act(f2 * f3)]
 *   mode 2: out = [act(a) | act(c) | act(f2) * act(f3)]  (mutag.py)       act: 0 = tanh, 1 = relu
 *   mode 3: out = [act(a) | act(c) | tanh(f2) * tanh(f3)]  (ptc.py:311: the factors always tanh, act on the first two parts)
 * w1, w2, w3: Linear weights [n, Fin] row-major, b*: [n] or NULL; wc: the SpectConv weight [Fin, n2]; val: one value per edge in the
 * order of `col` (NULL: ones, the scripts' torch.ones edge_attr).  Exact fp32 products.  Fin <= 144, n1, n2, n3 <= 64 (gml_gnnml1_supported),
 * else GML_E_UNSUPPORTED and the caller composes the block from gml_spectconv_fwd and library Linears.
 * Backward (source-keyed view rowptr_t / col_t / val_t; `out` = the saved forward output, gout = dL/dout):
 *   dx (optional) = da W1 + df2 W2 + df3 W3 + (A dc) Wc^T                    da, dc, df2, df3 = gradients at a, c, f2, f3
 *   g4 [N, ldg4 >= gml_gnnml1_g4_cols()] = [da | dc (modes 1 .. 3 only: dc = da in mode 0) | df2 | df3], each block 16 ceil(n / 16) columns wide
 *   q  [N, ldq >= 16 ceil(n2 / 16)]      = A dc
 * from which the caller forms dW1 = da^T x, dW2 = df2^T x, dW3 = df3^T x, dWc = x^T q (gml_xty) and the bias gradients (column sums). */
int gml_gnnml1_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode);
int gml_gnnml1_g4_cols(int32_t n1, int32_t n2, int32_t n3, int32_t mode);
int gml_gnnml1_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                   int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                   const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t mode, int32_t act,
                   float* out, int64_t ldo, gml_stream_t stream);
/* the block's weight and bias gradients from g4 / q in one pass over the rows + one fold:
 *   out_flat = [dW1 (n1 x Fin) | dW2 (n3 x Fin) | dW3 (n3 x Fin) | dWc (Fin x n2) | column sums of g4 (gml_gnnml1_g4_cols floats)]
 * (db1 = sums of the da block, dbc = sums of the dc block -- the da block in mode 0 --, db2 / db3 = sums of the df2 / df3 blocks) */
int64_t gml_gnnml1_dw_floats(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode);
size_t gml_gnnml1_dw_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode);
int gml_gnnml1_dw(const float* x, int64_t ldx, const float* g4, int64_t ldg4, const float* q, int64_t ldq, int64_t num_rows,
                  int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode, float* out_flat, void* ws, size_t ws_bytes,
                  gml_stream_t stream);
int gml_gnnml1_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, const float* x, int64_t ldx,
                   const float* out, int64_t ldo, const float* gout, int64_t ldgo, int64_t num_rows, int32_t Fin,
                   const float* w1, int32_t n1, const float* wc, int32_t n2, const float* w2, const float* b2, const float* w3,
                   const float* b3, int32_t n3, int32_t mode, int32_t act, float* dx, int64_t lddx, float* g4, int64_t ldg4,
                   float* q, int64_t ldq, gml_stream_t stream);

/* GNNML1 block in the sum-and-factors form (block mode 4; csrc/gml_gnnml1_sum.hip) -- enzymes_contfeat.py:284-346:
 *   out [N, n1 + n3] = [ act(a) + act(c) | act(f2) * act(f3) ],   a, c, f2, f3 and the arguments as for gml_gnnml1_fwd,  n1 == n2.
 * Fin <= 192, n1 = n2 <= 128, n3 <= 64 (gml_gnnml1_sum_supported), else GML_E_UNSUPPORTED; n1 != n2: GML_E_BADARG.  Rows of any stride;
 * exact fp32 products, aggregation in edge order, no atomics.  The weight image is split over the grid's second dimension by column
 * groups (64 columns of fc_i1 and conv_i1 each, one group for fc_i2 / fc_i3): at most 98,304 bytes of LDS per workgroup.
 * pattern (optional, [N, ldp >= 4 ceil(n1 / 16)] bytes): the forward records where a and c are positive -- byte j of a row: bit u = a > 0,
 * bit 4 + u = c > 0 of column 4 j + u -- because the sum does not tell the two relu patterns apart.
 * Backward: with the forward's pattern (act = 1 only, else GML_E_BADARG) da and dc come from gout and the bits; with pattern = NULL
 * (tanh needs the values) a and c are RECOMPUTED from x over the TARGET-keyed view (rowptr / col / val, as the forward).  f2, f3 are
 * always recomputed; no forward output is read.  q and dx use the SOURCE-keyed view (rowptr_t / col_t / val_t):
 *   g4 [N, ldg4 >= gml_gnnml1_sum_g4_cols()] = [da | dc | df2 | df3],  da = g act'(a), dc = g act'(c); each part 16 ceil(n / 16) wide
 *   q  [N, ldq >= 16 ceil(n1 / 16)] = A dc;      dx (optional) = da W1 + q Wc^T + df2 W2 + df3 W3
 * g4, q: 16-byte aligned, ldg4 and ldq multiples of 4.  gml_gnnml1_sum_dw: all weight gradients and the column sums of g4 (the bias
 * gradients) in one pass over the rows + one ordered fold:
 *   out_flat = [dW1 (n1 x Fin) | dW2 (n3 x Fin) | dW3 (n3 x Fin) | dWc (Fin x n2) | column sums of g4 (gml_gnnml1_sum_g4_cols floats)] */
int gml_gnnml1_sum_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3);
int gml_gnnml1_sum_g4_cols(int32_t n1, int32_t n2, int32_t n3);
int gml_gnnml1_sum_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                       int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                       const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                       float* out, int64_t ldo, uint8_t* pattern, int64_t ldp, gml_stream_t stream);
int gml_gnnml1_sum_bwd(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* rowptr_t, const int32_t* col_t,
                       const float* val_t, const float* x, int64_t ldx, const float* gout, int64_t ldgo, int64_t num_rows,
                       int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                       const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                       const uint8_t* pattern, int64_t ldp, float* dx, int64_t lddx, float* g4, int64_t ldg4, float* q, int64_t ldq,
                       gml_stream_t stream);
int64_t gml_gnnml1_sum_dw_floats(int32_t Fin, int32_t n1, int32_t n2, int32_t n3);
size_t gml_gnnml1_sum_dw_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t n1, int32_t n2, int32_t n3);
int gml_gnnml1_sum_dw(const float* x, int64_t ldx, const float* g4, int64_t ldg4, const float* q, int64_t ldq, int64_t num_rows,
                      int32_t Fin, int32_t n1, int32_t n2, int32_t n3, float* out_flat, void* ws, size_t ws_bytes,
                      gml_stream_t stream);

/* GNNML1 block as the sum of three activated parts (block mode 5; csrc/gml_gnnml1_act.hip) -- filtering.py:246-248 (concat = False):
 *   out [N, n] = act(a) + act(c) + act(f2 * f3),   a, c, f2, f3 and the arguments as for gml_gnnml1_fwd,  n1 == n2 == n3 == n.
 * One launch forward, the kernel of gml_gnnml1_fwd with another epilogue: exact fp32 products, aggregation in edge order, no atomics.
 * act = 1 (relu), Fin <= 144, n <= 64 (gml_gnnml1_actsum_supported), else GML_E_UNSUPPORTED -- act = 0 (tanh) included: it needs the
 * values of a and c in the backward, no script uses it in this form, and the caller composes it; unequal widths or an act outside
 * 0 / 1: GML_E_BADARG.  Nothing is launched on any error.  Rows of any stride.
 * pattern ([N, ldp >= 4 ceil(n / 16)] bytes; optional in the forward): where a and c are positive -- byte j of a row: bit u = a > 0,
 * bit 4 + u = c > 0 of column 4 j + u (the layout of gml_gnnml1_sum_fwd) -- because the sum does not tell the relu patterns apart.
 * Backward (source-keyed view rowptr_t / col_t / val_t; pattern required, NULL: GML_E_BADARG; no forward output is read):
 *   g4 [N, ldg4 >= gml_gnnml1_g4_cols(n, n, n, 1)] = [da | dc | df2 | df3],  da = g [a > 0], dc = g [c > 0],
 *                                                     df2 = g [f2 f3 > 0] f3, df3 = g [f2 f3 > 0] f2  (f2, f3 recomputed; relu'(0) = 0)
 *   q  [N, ldq >= 16 ceil(n / 16)] = A dc;      dx (optional) = da W1 + q Wc^T + df2 W2 + df3 W3
 * ldg4 and ldq multiples of 4; padding columns of g4 are zeros.  g4 is mode 1's layout: the weight and bias gradients come from
 * gml_gnnml1_dw(..., mode = 1) (workspace: gml_gnnml1_dw_workspace_bytes(..., mode = 1)). */
int gml_gnnml1_actsum_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t act);
int gml_gnnml1_actsum_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                          int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                          const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                          float* out, int64_t ldo, uint8_t* pattern, int64_t ldp, gml_stream_t stream);
int gml_gnnml1_actsum_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, const float* x, int64_t ldx,
                          const float* gout, int64_t ldgo, int64_t num_rows, int32_t Fin, const float* w1, int32_t n1,
                          const float* wc, int32_t n2, const float* w2, const float* b2, const float* w3, const float* b3,
                          int32_t n3, int32_t act, const uint8_t* pattern, int64_t ldp, float* dx, int64_t lddx,
                          float* g4, int64_t ldg4, float* q, int64_t ldq, gml_stream_t stream);

/* PPGN (the 3-WL baseline of every experiment script, e.g. sr25.py:20-72) on dense channel-major tensors [B, C, nmax, nmax]
 * (csrc/gml_ppgn.hip).  n [B] int32: the node counts; pixel (i, j) of graph g is real where i < n_g and j < n_g (mask m).
 *
 * gml_ppgn_inputs: the tensors of libs/utils.py:613-624 for a batch, one launch, no host read.  X2 [B, nfeat + 2, nmax, nmax] and
 * M [B, 2, nmax, nmax] must arrive ZERO FILLED; the kernel sets X2 channel 0 = adjacency (edge (s, d) -> pixel (s, d) of the graph of
 * s), channel 1 = identity on the first n_g diagonal entries, channel 2 + f = diag(x[:, f]) for f < nfeat <= ldx; M channel 0 = the
 * diagonal mask, channel 1 = the off-diagonal mask inside n_g x n_g; n [B] = ptr[g + 1] - ptr[g].  A graph with n_g > nmax gets no
 * pixel at all (its n is still written: the caller's check).  edge_src / edge_dst: global node ids (int64), batch [N]: graph of a node.
 *
 * gml_ppgn_fwd: one block,
 *   a1 = relu(m (W1 x + b1)),  a2 = relu(m (W2 x + b2)),  p_c = a1_c @ a2_c per channel,  y = relu(m (W3 [p ; x] + b3))
 *   W1, W2 [C, Cin], W3 [C, C + Cin] row-major (first C columns on p), biases optional (NULL).  Three launches.
 *   a12 [B, 2C, nmax, nmax] (a1 then a2) and p [B, C, nmax, nmax] are written on the real pixels only (the backward's inputs; the
 *   padding is never read), y [B, C, nmax, nmax] everywhere (exactly 0 in the padding, whatever x holds there).
 *   r: the layer readout out of the kernel that writes y.  r0_c = sum_i y_c[i, i], r1_c = sum_{i != j} y_c[i, j];
 *   readout 0 ('sum'): r [B, 2C] = [r0 | r1];  1 ('mean'): [r0 / n | r1 / (n^2 - n)] (n = 1: 0 / 0, the reference's arithmetic);
 *   2 ('diag'): r [B, C] = r0.
 * gml_ppgn_bwd: dy [B, C, nmax, nmax] and / or dr (shape of r); either may be NULL, not both.  Four launches + one for dx (optional,
 *   [B, Cin, nmax, nmax], exactly 0 in the padding).  Relu patterns from y > 0 and a > 0.  Weight and bias gradients: per-workgroup
 *   partials over 32-pixel chunks on the f32-input matrix instruction, then one fold in ascending workgroup order (no atomics:
 *   bit-reproducible).  dflat [gml_ppgn_dw_floats] = [D3 (C x (C + Cin + 1)) | D12 (2C x (Cin + 1))] row-major:
 *   D3 = [dW3 | db3], D12 = [dW1 | db1 ; dW2 | db2] (the bias column is computed with or without biases).
 * Range: 1 <= nmax <= 64, 1 <= Cin, C <= 64 (gml_ppgn_supported), else GML_E_UNSUPPORTED; nothing is launched on any error.
 * Exact fp32 products and sums throughout.  No host synchronisation: capturable on one stream. */
int gml_ppgn_supported(int32_t nmax, int32_t Cin, int32_t C);
int gml_ppgn_inputs(const float* x, int64_t ldx, int32_t nfeat, const int64_t* edge_src, const int64_t* edge_dst, int64_t E,
                    const int32_t* ptr, const int64_t* batch, int64_t N, int64_t B, int32_t nmax, float* X2, float* M, int32_t* n,
                    gml_stream_t stream);
int gml_ppgn_fwd(const float* x, const int32_t* n, int64_t B, int32_t nmax, int32_t Cin, int32_t C, const float* w1, const float* b1,
                 const float* w2, const float* b2, const float* w3, const float* b3, int32_t readout, float* a12, float* p, float* y,
                 float* r, gml_stream_t stream);
int64_t gml_ppgn_dw_floats(int32_t Cin, int32_t C);
size_t gml_ppgn_bwd_workspace_bytes(int64_t B, int32_t nmax, int32_t Cin, int32_t C);
int gml_ppgn_bwd(const float* x, const int32_t* n, int64_t B, int32_t nmax, int32_t Cin, int32_t C, const float* w1, const float* w2,
                 const float* w3, const float* a12, const float* p, const float* y, const float* dy, const float* dr, int32_t readout,
                 float* dx, float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream);

/* GAT (the attention baseline of every PyG experiment script, e.g. Zinc12k.py:221-245): the edge-softmax attention of GATConv
 * (torch_geometric 1.6.1, concat=True, negative_slope 0.2, no attention dropout) behind the projection xl = x W^T, which the caller
 * computes (csrc/gml_gat.hip).  xl [N, H C] in rows of ldxl, head h = columns [h C, (h + 1) C).  The graph is a GraphCSR's two views:
 * (rowptr, col) lists the sources j of every target i, (rowptr_t, col_t) the targets i of every source j, pos_t[k] = the target-view
 * position of source-view edge k.  Entries with col == row are skipped and ONE self edge per node is implicit; repeated edges count
 * once per occurrence.
 *
 * gml_gat_logits: al[n, h] = sum_c xl[n, h, c] att_l[h, c] (the source term), ar likewise with att_r (the target term); al, ar [N, H]
 *   contiguous, c ascending.  One launch.
 * gml_gat_fwd: per target i and head h over its edges (j -> i), the self edge first, then the row in CSR order:
 *   s = al[j, h] + ar[i, h],  e = s > 0 ? s : 0.2 s,  m = max e,  p = exp(e - m),  z = sum p,  out = (sum p xl[j, h, :]) / (z + 1e-16)
 *   y[i] = act(out + bias), act 0 none / 1 relu / 2 tanh / 3 elu (alpha = 1); bias [H C] optional (NULL).  Two passes over the row (max,
 *   then sums), so rows of any degree are served.  m, z [N, H] contiguous: the backward's inputs.  One launch.
 * gml_gat_bwd: dy [N, H C] in rows of lddy -> dxl [N, H C] (rows of lddxl), datt_l, datt_r [H C], dbias [H C] (optional, NULL).
 *   g = dy act'(y) (act' from y alone).  Four launches:
 *   target view : g, d_e = <g[i, h], xl[j, h] - xl[i, h]> per edge and head (= dalpha_e - dalpha_self: the softmax gradient does not
 *                 change under a shift of dalpha, and the differences keep their digits where neighbouring rows are alike) to the
 *                 workspace in target-view order, S[i, h] = sum_e alpha_e d_e (= <g, out - xl[i]>), dar[i, h] = sum_e slope_e alpha_e
 *                 (d_e - S) as sum slope alpha d - S sum slope alpha in the same pass, alpha recomputed from al, ar, m, z
 *   source view : ds_e = slope_e alpha_e (d_e - S[i, h]) where it is used; dal[j, h] = sum over the edges out of j of ds_e;
 *                 dxl[j, h, :] = sum_e alpha_e g[i, h, :] + dal[j, h] att_l[h, :] + dar[j, h] att_r[h, :]   (self edge first, then CSR order)
 *   reduction   : per-workgroup partials of datt_l = sum_n dal[n, h] xl[n, h, c], datt_r (with dar) and dbias = sum_n g over
 *                 contiguous row ranges, n ascending; then one fold in ascending workgroup order.
 *   No atomics: every sum has a fixed order, two runs give the same bits.
 * Range: H = 8, C in {4, 8, 12, 16, 32} (gml_gat_supported), any N >= 1, E >= 0 (below 2^31), any degree; rows must be float4
 * addressable (pointers 16-byte aligned, leading dimensions multiples of 4), else GML_E_UNSUPPORTED.  Nothing is launched on any error.
 * Plain fp32 fmaf / expf / tanhf.  No allocation, no host read: capturable on one stream. */
int gml_gat_supported(int32_t H, int32_t C);
int gml_gat_logits(const float* xl, int64_t ldxl, const float* att_l, const float* att_r, int64_t N, int32_t H, int32_t C, float* al,
                   float* ar, gml_stream_t stream);
int gml_gat_fwd(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldxl, const float* al, const float* ar,
                const float* bias, int64_t N, int64_t E, int32_t H, int32_t C, int32_t act, float* y, int64_t ldy, float* m, float* z,
                gml_stream_t stream);
size_t gml_gat_bwd_workspace_bytes(int64_t N, int64_t E, int32_t H, int32_t C);
int gml_gat_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* pos_t,
                const float* xl, int64_t ldxl, const float* al, const float* ar, const float* m, const float* z, const float* y,
                int64_t ldy, const float* dy, int64_t lddy, const float* att_l, const float* att_r, int64_t N, int64_t E, int32_t H,
                int32_t C, int32_t act, float* dxl, int64_t lddxl, float* datt_l, float* datt_r, float* dbias, void* ws,
                size_t ws_bytes, gml_stream_t stream);

/* GIN (the 1-WL baseline of every PyG experiment script, e.g. Zinc12k.py:97-143, sr25.py:74-105): GINConv of torch_geometric 1.6.1
 * with its nn = Sequential(Linear) (depth 1) or Sequential(Linear, ReLU, Linear) (depth 2) and the script's activation in one launch
 * (csrc/gml_gin.hip).  (rowptr, col) lists the sources j of every target i (a GraphCSR's target view), (rowptr_t, col_t) the targets
 * of every source.  EVERY edge occurrence counts, a self loop included; nothing is dropped or added.
 *
 * gml_gin_fwd: per target row i
 *     h[i] = sum over the row's edges (j -> i) in CSR order of x[j], then + (1 + eps) x[i]          (this order is the contract)
 *     depth 2: t = relu(W1 h + b1) [N, Fh], y = act(W2 t + b2) [N, Fout];   depth 1: y = act(W1 h + b1) [N, Fh]
 *   act 0 none / 1 relu / 2 tanh; w1 [Fh, Fin], w2 [Fout, Fh] dense row-major; b1, b2 optional (NULL).  eps is a DEVICE pointer to
 *   one float, read inside the kernel: a captured launch sees the optimiser's update on replay.  h (rows of ldh) and, at depth 2, t
 *   (rows of ldt) are the backward's inputs.  With depth 1, w2, b2, t, ldt and Fout are not read.  Products: the bias first, then k
 *   ascending fmaf.  Rows are chunked: any degree.  ONE launch.
 * gml_gin_bwd: dy (rows of lddy) -> dx (rows of lddx; NULL: not wanted, the source view is not walked) and
 *   dflat = [dW1 Fh x Fin | db1 Fh | dW2 Fout x Fh | db2 Fout (depth 2 only) | deps 1], gml_gin_dflat_floats floats.
 *     g2 = dy act'(y) (act' from y alone);  depth 2: dW2 = g2^T t, db2 = sum g2, g1 = (g2 W2) [t > 0];  depth 1: g1 = g2
 *     dW1 = g1^T h, db1 = sum g1, dh = g1 W1, deps = sum_i <dh[i], x[i]>
 *     dx[j] = (1 + eps) dh[j], then + dh[i] over the edges (j -> i) in source-view CSR order
 *   THREE launches (TWO with dx == NULL): the row pass (per-workgroup partials of dflat over contiguous row ranges, rows ascending;
 *   dh to the workspace), the source-view aggregation, the fold of the partials in ascending workgroup order.  No atomics: every sum
 *   has a fixed order, two runs give the same bits.
 * Range: depth in {1, 2}, 1 <= Fin, Fh, Fout <= 64 (gml_gin_supported; Fout is not read at depth 1), any N >= 1, E >= 0 (below
 * 2^31), any degree, rows of any stride >= their width (no alignment beyond a float's); else GML_E_UNSUPPORTED.  A workspace below
 * gml_gin_bwd_workspace_bytes: GML_E_WORKSPACE.  Nothing is launched on any error.  Plain fp32 fmaf / tanhf.  No allocation, no host
 * read: capturable on one stream. */
int gml_gin_supported(int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth);
int gml_gin_fwd(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, int64_t N, int64_t E, int32_t Fin, const float* eps,
                const float* w1, const float* b1, int32_t Fh, const float* w2, const float* b2, int32_t Fout, int32_t depth, int32_t act,
                float* h, int64_t ldh, float* t, int64_t ldt, float* y, int64_t ldy, gml_stream_t stream);
int64_t gml_gin_dflat_floats(int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth);
size_t gml_gin_bwd_workspace_bytes(int64_t N, int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth);
int gml_gin_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* x, int64_t ldx, const float* h, int64_t ldh, const float* t,
                int64_t ldt, const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t N, int64_t E, int32_t Fin, const float* eps,
                const float* w1, int32_t Fh, const float* w2, int32_t Fout, int32_t depth, int32_t act, float* dx, int64_t lddx,
                float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream);

/* ChebNet (the spectral baseline of every PyG experiment script, e.g. Zinc12k.py:193-219, sr25.py:149-167): ChebConv(Fin, Fout, K) of
 * torch_geometric 1.6.1 with normalization 'sym' and the script's activation (csrc/gml_cheb.hip).  (rowptr, col) lists the sources j of
 * every target i (a GraphCSR's target view), (rowptr_t, col_t) the targets of every source.  Self loops are dropped; every other edge
 * occurrence counts, duplicates included.  The graph need not be symmetric.
 *
 * gml_cheb_norm: norm [N][2] = (dis[i], s[i]), ONE launch per batch, shared by every layer of a model.
 *     deg[i] = the non-self edges of the SOURCE row i with a target in [0, N);  dis[i] = 1 / sqrt(deg[i]), 0 at deg 0
 *     s[i] = 2 / lmax[batch[i]]  (lmax [B] and batch [N], int32, DEVICE pointers; batch NULL: graph 0; a graph id outside [0, B): 2.0),
 *            or 2 / lambda for every row when lmax == NULL.  lmax <= 0 or not finite is outside the contract (nothing reads it on host).
 *   The scaled Laplacian it stands for:  L^[i, j] = sum over the edges (j -> i, j != i) of w,  w = (-(s[i] dis[i])) dis[j]  (two fp32
 *   products in this order),  L^[i, i] = s[i] - 1, for isolated rows too.
 * gml_cheb_fwd: Tx_0 = x, Tx_1 = L^ x, Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2};  y = act(bias + sum_k Tx_k W_k)
 *   act 0 none / 1 relu / 2 tanh; w [K][Fin][Fout] dense row-major; bias [Fout] optional (NULL).  T [N, (K - 1) Fin] (rows of ldT)
 *   receives Tx_1 .. Tx_{K-1} side by side: the backward's inputs (Tx_0 = x is not copied; T is not read at K = 1).  y doubles as the
 *   accumulator between the launches.  K - 1 launches (each step needs the neighbours' previous Tx), ONE at K = 1.
 *   The orders are the contract:
 *     a Tx_k element  a = 0; the row's edges in CSR order: a = fmaf(w, Tx_{k-1}[j][c], a); then a = fmaf(s[i] - 1, Tx_{k-1}[i][c], a);
 *                     k = 1: Tx_1 = a;  k >= 2: Tx_k = fmaf(2, a, -Tx_{k-2}[i][c])
 *     a y element     acc = bias (0 without one); then k = 0 .. K - 1 ascending, inside k the input column c ascending:
 *                     acc = fmaf(Tx_k[i][c], W_k[c][o], acc);  y = act(acc)
 * gml_cheb_bwd: dy (rows of lddy) -> dx (rows of lddx; NULL: not wanted, the adjoint steps are skipped) and
 *   dflat = [dW_0 .. dW_{K-1}, each Fin x Fout | db Fout], gml_cheb_dflat_floats floats.  With g = dy act'(y) (act' from y alone):
 *     dW_k = Tx_k^T g,  db = sum_i g[i],  G_{K-1} = g W_{K-1}^T,  G_k = g W_k^T + c_k L^T G_{k+1} - G_{k+2} (c_0 = 1, else 2; terms with
 *     an index above K - 1 absent),  dx = G_0.  L^T walks the SOURCE view with the forward's w of every edge.
 *     a G_k element   a = 0; the source row's edges in CSR order: a = fmaf(w, G_{k+1}[i][c], a); then a = fmaf(s[j] - 1, G_{k+1}[j][c], a);
 *                     p = 0, o ascending: p = fmaf(g[j][o], W_k[c][o], p);  G_k = fmaf(c_k, a, p), then - G_{k+2}[j][c]
 *   Launches: the row pass (per-workgroup partials of dflat over contiguous row ranges, rows ascending, k ascending inside a tile of
 *   32 rows; it also forms g W_{K-1}^T: dx at K = 1), K - 1 adjoint steps (three rotating [N, Fin] buffers in the workspace; the last
 *   writes dx), the fold of the partials in ascending workgroup order: K + 1 launches, TWO with dx == NULL.  No atomics: two runs give
 *   the same bits.
 * Range: 1 <= K <= 8, 1 <= Fin, Fout <= 64 (gml_cheb_supported), any N >= 1, E >= 0 (below 2^31), any degree, rows of any stride >=
 * their width (no alignment beyond a float's); else GML_E_UNSUPPORTED.  A workspace below gml_cheb_bwd_workspace_bytes:
 * GML_E_WORKSPACE.  Nothing is launched on any error.  Column ids outside [0, N) are skipped.  Plain fp32 fmaf / tanhf.  No allocation,
 * no host read: capturable on one stream. */
int gml_cheb_supported(int32_t Fin, int32_t Fout, int32_t K);
int gml_cheb_norm(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* batch, const float* lmax, int64_t B, float lambda,
                  int64_t N, int64_t E, float* norm, gml_stream_t stream);
int gml_cheb_fwd(const int32_t* rowptr, const int32_t* col, const float* norm, const float* x, int64_t ldx, int64_t N, int64_t E,
                 int32_t Fin, const float* w, const float* bias, int32_t Fout, int32_t K, int32_t act, float* T, int64_t ldT, float* y,
                 int64_t ldy, gml_stream_t stream);
int64_t gml_cheb_dflat_floats(int32_t Fin, int32_t Fout, int32_t K);
size_t gml_cheb_bwd_workspace_bytes(int64_t N, int32_t Fin, int32_t Fout, int32_t K);
int gml_cheb_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* norm, const float* x, int64_t ldx, const float* T, int64_t ldT,
                 const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t N, int64_t E, int32_t Fin, const float* w, int32_t Fout,
                 int32_t K, int32_t act, float* dx, int64_t lddx, float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GML_H_ */
