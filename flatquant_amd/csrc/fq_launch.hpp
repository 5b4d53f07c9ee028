// fq_launch.hpp — the launchers: every host function one translation unit of libfqhip.so calls in another. The kernel files define
// them, fq_capi.hip (and a kernel file that routes to another's kernels) calls them, and all of them include this header, so a
// definition that disagrees with its declaration does not compile. Default arguments are given here and nowhere else.
// The launchers are ordinary external functions: an FQHIP_OVERLAY build (tools/variants.sh) replaces them through the PLT.
#pragma once
#include "fq_common.hpp"

// What a launcher returns besides a hipError_t (0 = launched): fq_capi.hip turns them into FQ_EUNSUPPORTED / FQ_EINVAL.
constexpr int FQ_LAUNCH_NO_KERNEL = -1000;   // no kernel is compiled for this flag combination / shape
constexpr int FQ_LAUNCH_NEED_WS = -1001;     // the launch needs a (larger) workspace

// ---- Kronecker transform + quantiser ----
// WHICH kernel a launch runs is decided in one place, fq_kron_route (fq_kron_route.hpp, included here: the instantiation lists, the
// order of preference, the shared preconditions). fq_launch_kron runs a route's kernel; the family launchers below it launch the
// instantiation they are handed and return FQ_LAUNCH_NO_KERNEL only for one that is not in their list.
#include "fq_kron_route.hpp"
int fq_launch_kron64(int k64_flags, int bf16_dtype, const void* x, const void* left, const void* right, const void* diag, int64_t rows,
                     const FqQuantOut& out, int n_cu, hipStream_t stream, const void* prep = nullptr);
int fq_launch_kron64_prepare(const void* left, const void* right, void* image, hipStream_t stream);
int fq_launch_kron64_linear(const f16* x, const void* prep, int64_t M, float rms_eps, bool rms, int rt_flags, int n, const void* const* wimg,
                            const f16* const* scol, const f16* const* bias, const float* sig_max, const float* sig_min, const int* N,
                            f16* const* y, int n_cu, hipStream_t stream);
int fq_launch_kron64_multi(int bf16_dtype, const void* jobs, int n_jobs, int bpj, const FqQuantOut& out, hipStream_t stream);
int fq_launch_kron64_trace(const f16* x, const f16* left, const f16* right, int64_t rows, const FqQuantOut& out,
                           unsigned long long* trace, int n_cu, hipStream_t stream);
// The optional workspace of the 64 x 64 pair: the 16 KB fragment image fq_kron64_kernel reads, followed by the 16 KB image of the
// workgroup-per-token kernel (the few output sets fq_kron64 has no instantiation for fall through to it).
constexpr int64_t FQ_K64_IMAGE_BYTES = 16384, FQ_K64_WS_BYTES = 32768;
int64_t fq_kron_generic_workspace_bytes(int M, int N);
int fq_launch_kron_prepare(const f16* left, const f16* right, int M, int N, void* workspace, hipStream_t stream, int groups = 1);
// fq_kron_route (without the 64 x 64 kernel), the fragment image unless FQ_WS_PREPARED, the launch. -> 0, a hipError_t, FQ_LAUNCH_NO_KERNEL / _NEED_WS.
int fq_launch_kron_generic(int flags, const f16* x, const f16* left, const f16* right, const f16* diag,
                           int64_t rows, int M, int N, const FqQuantOut& out, void* workspace,
                           int64_t workspace_bytes, int n_cu, hipStream_t stream);
int fq_launch_kron(const FqKronRoute& r, int flags, const f16* x, const f16* left, const f16* right, const f16* diag, int64_t rows, int M, int N,
                   const FqQuantOut& out, void* workspace, int n_cu, hipStream_t stream);   // (the same after a route of the caller's)
int fq_launch_kron_grouped_mats(int flags, const void* x, const void* left, const void* right, int64_t rows, int M, int N,
                                const FqQuantOut& out, int n_groups, void* workspace, int64_t workspace_bytes, int n_cu,
                                hipStream_t stream);
// the kernel families: r = the route (its family's); a.flags = the output set and run-time bits, x / diag = f16 or bf16 as r says, ws = the fragment image
struct FqKronArgs {
    int flags;
    const void *x, *ws, *diag;
    int64_t rows;
    int M, N, n_cu;
    hipStream_t stream;
};
int fq_launch_kron_wave(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);
int fq_launch_kron_tiles(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);
int fq_launch_kron_trio(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);
int fq_launch_kron_duo(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);
int fq_launch_kron_tall(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);
int fq_launch_kron_fast(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);    // (f16: fq_kron_generic.hip)
int fq_launch_kron_fast2(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);   // (bf16, group-128: fq_kron_generic2.hip)
int fq_launch_kron_general(const FqKronRoute& r, const FqKronArgs& a, const FqQuantOut& out);

// ---- block-diagonal transform, Hadamard, row quantisers, elementwise ----
int fq_launch_block(int flags, const f16* x, const f16* P, int64_t rows, int R, int C, int transpose_out,
                    const FqQuantOut& out, int n_cu, hipStream_t stream);
int fq_launch_block_linear(const f16* x, const f16* P, int64_t M, int R, int C, float sig_max, float sig_min, int rt_flags, const void* wimg,
                           const f16* scol, const f16* bias, int N, f16* y, int n_cu, hipStream_t stream);
int fq_launch_hadamard(const f16* x, f16* y, int64_t rows, int n, int K, const f16* hadK, float scale,
                       int n_cu, hipStream_t stream);
int fq_launch_hadamard_reg(const f16* x, f16* y, int64_t rows, int n, int K, const f16* hadK, float scale, int n_cu,
                           hipStream_t stream);
int fq_launch_fwht_f32(const f16* x, float* y32, int64_t vecs, int P, float scale, int n_cu, hipStream_t stream);
int fq_launch_had_mfma(const f16* x, int64_t rows, int n, int K, const f16* hadK, float scale, float sig_max, float sig_min,
                       uint8_t* q_out, f16* scale_out, f16* y_out, int n_cu, hipStream_t stream, const f16* up = nullptr,
                       int plain_quantizer = 0);
int fq_launch_hadamard_quant(const f16* x, int64_t rows, int n, int K, const f16* hadK, float scale, float sig_max,
                             float sig_min, uint8_t* q, f16* scale_out, int n_cu, hipStream_t stream);
int fq_launch_silu_hadamard_quant(const f16* gate, const f16* up, int64_t rows, int n, int K, const f16* hadK, float scale,
                                  float sig_max, float sig_min, uint8_t* q, f16* scale_out, int n_cu, hipStream_t stream);
int fq_launch_rowquant(int flags, const f16* x, int64_t rows, int cols, const FqQuantOut& out, int n_cu,
                       hipStream_t stream);
int fq_launch_fakequant_bits(int bf16_dtype, const void* x, void* y, int64_t rows, int cols, float sig_max, float sig_min, int bits, int flags,
                             int n_cu, hipStream_t stream);
int fq_launch_sym_quant(const f16* x, const f16* scale, int64_t rows, int cols, uint8_t* q, int n_cu,
                        hipStream_t stream);
int fq_launch_sym_dequant(const int32_t* q, const f16* srow, const f16* scol, int64_t rows, int cols,
                          f16* x, int n_cu, hipStream_t stream);
int fq_launch_silu_mul(const f16* gate, const f16* up, f16* y, int64_t n, int n_cu, hipStream_t stream);
int fq_launch_rmsnorm(const f16* x, f16* y, int64_t rows, int cols, float eps, int n_cu, hipStream_t stream);
int fq_launch_rowmm(int bf16_dtype, const void* x, const void* Tm, void* y, int64_t rows, int n, int n_cu, hipStream_t stream);
int fq_launch_rope(f16* q_out, f16* k_out, const f16* q, const f16* k, const f16* cos, const f16* sin, int64_t tokens, int q_heads, int k_heads,
                   int head_dim, hipStream_t stream);

// ---- GEMMs ----
int fq_launch_gemm_i4(const uint8_t* X, const uint8_t* W, int64_t M, int N, int K, int32_t* c, f16* y, const f16* srow,
                      const f16* scol, const f16* bias, hipStream_t stream);
// every expert's GEMM as one launch (fq_gemm_i4_grouped.hip): rows sorted by group, w / scol / bias stacked per group, offsets on the device
int fq_launch_gemm_i4_grouped(const uint8_t* X, const uint8_t* Wg, int64_t rows, int N, int K, const int64_t* group_offsets, int n_groups,
                              int32_t* c, f16* y, const f16* srow, const f16* scol_g, const f16* bias_g, hipStream_t stream);
int64_t fq_i4_frag_bytes(int N, int K);
int fq_launch_i4_to_frag(const uint8_t* W, int N, int K, void* img, int n_cu, hipStream_t stream);
int fq_launch_gemm_i4_skinny(const uint8_t* X, const void* wimg, int64_t M, int N, int K, int32_t* c, f16* y, const f16* srow,
                             const f16* scol, const f16* bias, hipStream_t stream);
int fq_launch_gemm_i4_skinny_multi(int n, const uint8_t* const* X, const void* const* wimg, int64_t M, const int* N, int K, f16* const* y,
                                   const f16* const* srow, const f16* const* scol, const f16* const* bias, hipStream_t stream);
int64_t fq_gemm_i4_skinny_split_ws_bytes(int64_t M, int N, int K);
int fq_launch_gemm_i4_skinny_split(const uint8_t* X, const void* wimg, int64_t M, int N, int K, f16* y, const f16* srow, const f16* scol,
                                   const f16* bias, int* kws, hipStream_t stream);
int64_t fq_bf6_blob_bytes(int64_t rows, int K);  // (exported as is)
int fq_launch_i4_to_bf6(const uint8_t* q, int64_t rows, int K, int perm, uint8_t* blob, int n_cu, hipStream_t stream);
int fq_launch_i4_to_bf6_multi(int nsrc, const uint8_t* const* q, int64_t rows, int K, int perm, uint8_t* blob, int n_cu, hipStream_t stream);
int fq_launch_gemm_bf6(const uint8_t* xblob, const uint8_t* wblob, int64_t M, int N, int K, int32_t* c, f16* y,
                       const f16* srow, const f16* scol, const f16* bias, hipStream_t stream);
int fq_launch_gemm_bf6_multi(int n, const uint8_t* const* xblob, const uint8_t* const* wblob, int64_t M, const int* Ns, int K, f16* const* y,
                             const f16* const* srow, const f16* const* scol, const f16* const* bias, hipStream_t stream);

// ---- K/V quantisers and the paged KV cache ----
int fq_launch_kv_quant(const f16* x, const f16* T, int64_t rows, int hd, float cmax, float cmin, bool lac, uint8_t* q,
                       f16* param, f16* y, int n_cu, hipStream_t stream);
int fq_launch_kv_dequant(const uint8_t* q, const f16* param, int64_t rows, int hd, bool lac, f16* y, int n_cu,
                         hipStream_t stream);
int64_t fq_kv_timage_bytes(int hd);
int fq_launch_kv_timage(const f16* T, int hd, void* img, hipStream_t stream);

// One layer of a paged cache as the host sees it. Every paged-cache launcher takes it and fills its own kernel-side struct from it
// (PagedKv, KvIO, ExtKv, CxArgs: their layouts are part of the kernels' tuned prologues and are not shared).
struct FqKvView {
    void* pages;                    // INT4 (or fp16) rows
    void* params;                   // (scale, zero) per row; unused with fp16 pages
    const int* indptr;
    const int* indices;
    const int* last_page_offset;
    int num_layers, layer_idx;
    int num_heads;                  // heads the CACHE holds
    int page_size, head_dim, batch;
    bool f16_pages;
};

// What an attention launch over the cache is asked to do. The cache serves num_heads / copies * share QUERY heads (q, o): `share`
// of them read one set of rows, and `copies` consecutive cache heads hold identical rows of which the first is read.
// copies = share = 1: the reference's layout read head by head; copies = 1, share = g: a cache that holds the KV heads once;
// copies = share = g: the reference's layout (g identical copies per KV head) read once per group.
struct FqKvAttn {
    f16* o;
    const f16* q;
    const f16* qt = nullptr;        // query transform [head_dim, head_dim], applied in the launch
    int transpose_out = 0;
    float* ws = nullptr;            // split workspace
    int splits = 1;                 // (decode: from fq_kv_decode_splits; the extend launches plan their own)
    int share = 1;
    int copies = 1;
    // decode only: the step's own row, quantised and appended by the launch (INT4 pages, head_dim 128, page_size % 16 == 0)
    const f16* k_new = nullptr;
    const f16* v_new = nullptr;
    const void* t_image = nullptr;  // fq_launch_kv_timage of the key transform
    int src_heads = 1;
    const f16* cos = nullptr;       // [batch, head_dim] rotary tables: the launch rotates its queries and the new K row first
    const f16* sin = nullptr;
    bool had = false;               // the normalised Hadamard rotation instead (had_scale = 1 / sqrt(head_dim)): no qt, image or tables
    float had_scale = 0.0f;
};

int fq_launch_kv_append(const FqKvView& c, const uint8_t* k, const uint8_t* v, const f16* kparam, const f16* vparam,
                        const int* seqlen_indptr, int64_t total_tokens, int group, int n_cu, hipStream_t stream);
int fq_launch_kv_quant_append(const FqKvView& c, const f16* k, const f16* v, const f16* T, int64_t tokens, int src_heads,
                              const float* clip4, bool lac, int added, int group, int n_cu, hipStream_t stream);
int fq_kv_decode_splits(int batch, int num_heads, int seq_hint);
int fq_kv_decode_wg_heads(int batch, int num_q_heads, int q_group, int head_dim);
int64_t fq_kv_decode_ws_bytes_gqa(int batch, int num_q_heads, int q_group, int head_dim);
int64_t fq_kv_decode_ws_bytes(int batch, int num_heads, int head_dim);
int fq_launch_kv_decode(const FqKvView& c, const FqKvAttn& a, hipStream_t stream);
int64_t fq_kv_extend_ws_bytes(int batch, int num_q_heads, int q_len, int head_dim);
int fq_launch_kv_extend(const FqKvView& c, const FqKvAttn& a, int q_len, int seq_hint, int64_t ws_bytes, hipStream_t stream);
int fq_launch_kv_chunk_extend(const FqKvView& c, const FqKvAttn& a, int q_len, hipStream_t stream);
int fq_launch_prefill_attn(f16* o, const f16* q, const f16* qt, const f16* k, const f16* v, const int* seq_start, const int* seq_len, int batch,
                           int seq, int q_heads, int kv_heads, hipStream_t stream);
