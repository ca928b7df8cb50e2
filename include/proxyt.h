/*
 * proxyt.h -- C ABI of libproxyt_hip.so, the MI355X (gfx950) implementation of
 * ProxyTransformation's point-cloud preshaping hot path.
 *
 * The reference has no native code and no FFI of its own (setup.py:108
 * ext_modules=[]); its native arithmetic is reached through pytorch3d / ATen.
 * Each entry point below names the reference interface it replaces, with
 * PRE = embodiedscan/models/necks/preshape_norm_reverse_drop.py.
 *
 * Conventions
 *   - every pointer is a CALLER-OWNED DEVICE pointer (HIP memory of the current
 *     device) unless marked [host]; the library never allocates or frees device
 *     memory; its only mutable state is a thread-local error string, the caller-owned PtxContext
 *     objects (side streams / events) and the optional per-kernel timing selection;
 *   - all tensors are dense, row-major, fp32 unless a type is given; index tensors
 *     are int32 on this side of the ABI (the reference's int64 -1-padded layout is
 *     kept: -1 = padding);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); work is only
 *     enqueued, no entry point synchronises the host;
 *   - return 0 on success, a negative PTX_E* code otherwise; ptx_last_error()
 *     returns a message for the calling thread.
 */
#ifndef PROXYT_H_
#define PROXYT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_ABI_VERSION 13

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY dynamic symbols
 * (tests/test_host_cpu.py::test_library_exports_every_declared_symbol asserts "these and nothing else"). */
#define PTX_API __attribute__((visibility("default")))

#define PTX_OK          0
#define PTX_EINVAL     -1   /* bad shape / null pointer / unsupported size */
#define PTX_ELAUNCH    -2   /* HIP launch or runtime error */
#define PTX_ENOSPACE   -3   /* workspace / prep buffer too small */
#define PTX_ETIMEOUT   -4   /* ptx_wait_counts: counts not published in time */
#define PTX_EGATE      -5   /* a stream gate of an earlier forward timed out (ptx_context_check, ptx_forward) */

/* Static shape of one forward (PRE:282-330 constructor values + input sizes). */
typedef struct PtxShape {
    int32_t B;          /* scenes in this call                                  */
    int32_t N;          /* points per scene (all equal: torch.cat at PRE:427)   */
    int32_t grid_size;  /* gs; M = gs^3 grid clusters (PRE:290)                 */
    int32_t K;          /* num_sub slots per cluster (PRE:291)                  */
    int32_t Mt;         /* M - int(0.3*M) clusters kept by padding count (PRE:374-376) */
    int32_t Mk;         /* int(M*(1-dynamic_drop_radio)) kept clusters (PRE:389)       */
    int32_t L;          /* text proxies                                          */
    int32_t V;          /* image proxies (views)                                 */
    int32_t C;          /* embed_dim (256)                                       */
    int32_t heads;      /* num_heads: 4, 8 (reference) or 16; head_dim 32 or 64   */
    int32_t hidden;     /* int(C*mlp_radio) (1024)                               */
    int32_t in_dim;     /* image feature channels (512)                          */
    int32_t hw;         /* img_spacial_dim^2 (225)                               */
    int32_t img_dtype;  /* storage type of img_feat: 0 = fp32, 1 = bf16, 2 = fp16 (AMP backbones);
                           arithmetic is fp32 in every case                      */
    float   radius;     /* 3.0 (PRE:23)                                          */
    float   margin;     /* 4.0 (PRE:23)                                          */
    float   bn_eps;     /* 1e-5                                                  */
    float   ln_eps;     /* 1e-5                                                  */
} PtxShape;

/* Conv2d(6,256,1)+BatchNorm2d(256) of OffsetNetwork / SimplifiedPointNet (PRE:72-76, 112-116). */
typedef struct PtxSlotMlp {
    const float *conv_w;   /* (256,6)  */
    const float *conv_b;   /* (256)    */
    const float *bn_w, *bn_b, *bn_mean, *bn_var;   /* (256) each, running stats */
} PtxSlotMlp;

/* One ProxyBlock + the LayerNorm applied after it (PRE:259-276, 441-443, 450-452). */
typedef struct PtxBlock {
    const float *norm1_w, *norm1_b;                 /* (C)                      */
    const float *pb_bias;                           /* (1,Mk,4,4)  PRE:199      */
    const float *pc_bias;                           /* (1,Mk,s,1)  PRE:200      */
    const float *pr_bias;                           /* (1,Mk,1,s)  PRE:201      */
    const float *qkv_w;                             /* (3C,C)      PRE:187      */
    const float *qkv_b;                             /* (3C) or NULL (qkv_bias=False) */
    const float *pp_w, *pp_b;                       /* proxy_proj (C,C),(C)     */
    const float *proj_w, *proj_b;                   /* (C,C),(C)                */
    const float *norm2_w, *norm2_b;                 /* (C)                      */
    const float *fc1_w, *fc1_b;                     /* (hidden,C),(hidden)      */
    const float *fc2_w, *fc2_b;                     /* (C,hidden),(C)           */
    const float *out_norm_w, *out_norm_b;           /* text_norm[i] / img_norm[i] */
} PtxBlock;

/* BatchNorm1d in eval mode (PRE:329-330). */
typedef struct PtxBn1d { const float *w, *b, *mean, *var; } PtxBn1d;

/* Raw reference-layout parameters: pointers straight into the nn.Module's storage. */
typedef struct PtxWeights {
    PtxSlotMlp   offset;            /* get_deformable_cluster.get_offsets.mlp     */
    const float *offset_map_w;      /* ...get_offsets.channel_mapper.weight (3,256) */
    PtxSlotMlp   encoder;           /* simple_encoder.mlp                         */
    const float *cm_w, *cm_b;       /* channel_mapper Conv2d(in_dim,C,1)  PRE:304 */
    const float *pos;               /* attn_pool2d.positional_embedding (hw+1,C)  */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *c_w, *c_b;   /* PRE:148-151 */
    const float *norm_img_w, *norm_img_b;
    PtxBlock     text;              /* textformer[-1] + text_norm[-1] */
    PtxBlock     img;               /* imgformer[-1]  + img_norm[-1]              */
    const float *text_trans_w, *text_trans_b;      /* Linear(C,3)  PRE:326       */
    const float *img_trans_w, *img_trans_b;        /* Linear(C,9)  PRE:327       */
    PtxBn1d      text_trans_norm, img_trans_norm;  /* PRE:329-330                */
} PtxWeights;

PTX_API int         ptx_abi_version(void);
PTX_API const char *ptx_last_error(void);

/* Library-owned streams and events of ONE caller (one nn.Module instance): the clustering chain and the
 * image chain of a forward run concurrently on private side streams that fork from / join into the
 * caller's stream.  Contexts are independent: two modules driven from two host threads on the same
 * device never share an event.  Create on the device the forwards will run on; destroy drains the side
 * streams first.  ptx_forward(ctx = NULL) uses a process-wide per-device default context and serialises
 * its enqueue section with a mutex. */
typedef struct PtxContext PtxContext;
PTX_API int ptx_context_create(PtxContext **ctx);
PTX_API int ptx_context_destroy(PtxContext *ctx);
/* Stream gates (ABI 6).  Where the image chain owns the caller's stream the fork and the join of the two chains are device
 * words instead of event record + wait (one waiting wave / one waiting work-group instead of two queue packets).  A waiter
 * is bounded in wall-clock time (PTX_GATE_TIMEOUT_MS, default 30 s for a fork, twice that for a join -- the fork legitimately waits for everything queued
 * ahead of the forward on the caller's stream); when the bound runs out it does NOT let go silently: it stores a sticky
 * error word in pinned host memory, the outputs of that forward become NaN, and (PTX_GATE_TRAP=1) it traps.
 * ptx_context_check returns PTX_EGATE once for such a failure -- ptx_forward makes the same check on entry -- and the
 * context orders its streams with events from then on.  The gates are used only after a probe per (context, caller
 * stream) has shown that the two streams run concurrently (they may share a hardware queue); PTX_GATE=0 / 1 forces
 * events / gates.  ptx_context_gates: nonzero while the context uses gates (bit 0; bit 1: its low-priority stream may carry
 * gate words as well).  There is no reference counterpart (PRE runs on
 * one stream). */
PTX_API int ptx_context_check(PtxContext *ctx);
/* ABI 11.  The same check BEHIND a drain of the context's streams and of the caller stream of its latest forward.  A join (or
 * slot-tag) gate fails after the survivor counts have been published, i.e. after a host that only waits for the counts has gone
 * on: ptx_context_check right behind ptx_wait_counts reports fork failures only, the join's surfaces with the NEXT
 * ptx_forward on the context -- or here.  Call it before trusting the outputs of forwards that were not synchronised on (end
 * of a loop, before results leave the process, at teardown); the Python module does so in check(), close() / __del__ and at
 * interpreter exit.  A C caller that sees PTX_EGATE must ptx_workspace_init its workspace again (the clean-on-entry words of
 * the failed forward cannot be trusted).  A fork's bound is PTX_GATE_TIMEOUT_MS (default 30 s: it covers everything the caller
 * queued ahead of the forward), a join's twice that (it may sit through a fork that runs into its bound).
 * Lifetime: the `stream` handle of the context's latest ptx_forward is synchronised here (and by the ptx_forward / ptx_context_check
 * that reports a failure): it must still be alive -- check BEFORE destroying a stream a forward was issued on.  A context that has
 * run no forward drains only its own streams. */
PTX_API int ptx_context_sync_check(PtxContext *ctx);
PTX_API int ptx_context_gates(const PtxContext *ctx);

/* Per-kernel timing of ptx_forward for roofline measurement (bench.py): select ONE launch
 * site by id (0 .. ptx_kernel_count()-1, -1 = off); every later ptx_forward brackets that
 * launch with HIP events recorded on the stream the kernel runs on.  ptx_timing_read()
 * waits for the recorded events and returns launches and summed milliseconds [host pointers],
 * then clears the record.  Do not enable while a stream capture is active. */
PTX_API int         ptx_kernel_count(void);
PTX_API const char *ptx_kernel_name(int kid);
PTX_API int         ptx_timing_select(int kid);
PTX_API int         ptx_timing_read(int *launches, float *total_ms);
/* Time only every n-th launch of a selected site (default 1 = every launch): an event record is a packet of its own and costs
 * the stream ~6 us of idle between the two kernels around it. */
PTX_API int         ptx_timing_every(int n);
/* Several launch sites at once (bit k of `mask` = site k); ptx_timing_read_sites fills two [host] arrays of
 * ptx_kernel_count() entries.  The event records perturb the step a little: use the single-site form inside a
 * timed region and the mask form for per-pass breakdowns. */
PTX_API int         ptx_timing_select_mask(uint64_t mask);
PTX_API int         ptx_timing_read_sites(int *launches, float *total_ms, int n);

/* Bytes of the parameter-only tables derived once per set of weights (folded
 * BatchNorm scale/shift, per-slot bias tables PRE:212-215, folded attention-pool
 * matrices) and of the per-call scratch.  Both buffers are caller-owned. */
PTX_API size_t ptx_prep_bytes(const PtxShape *s);
PTX_API size_t ptx_workspace_bytes(const PtxShape *s);

/* A workspace must be initialised ONCE after allocation (and again after a failed ptx_forward): ptx_forward finds
 * the ownership tags, encoded bounding boxes and count accumulators zero and its kernels leave them zero -- there
 * is no clearing launch on the per-call path. */
PTX_API int ptx_workspace_init(const PtxShape *s, void *workspace, size_t ws_bytes, void *stream);

/* Build the derived tables in `prep`.  lin = torch.linspace(0,1,gs) (gs floats, device);
 * it is uploaded by the caller because torch's two-sided linspace formula is part of
 * the reference's arithmetic (PRE:41).  Re-run after any parameter changes. */
PTX_API int ptx_prepare(const PtxShape *s, const PtxWeights *w, const float *lin,
                void *prep, size_t prep_bytes, void *stream);

/* ------------------------------------------------------------------ stage entry points
 * Each mirrors one reference function so it can be parity-tested on its own. */

/* PRE:37-48 init_uniform_cluster_center: per-scene min/max + gs^3 grid centres.
 * minmax (B,2,3): [b][0]=min, [b][1]=max.  centers (B,M,3). */
PTX_API int ptx_grid_centers(const float *points, int B, int N, const float *lin, int gs, float margin,
                     float *minmax, float *centers, void *workspace, size_t ws_bytes, void *stream);

/* pytorch3d.ops.ball_query(p1=centers, p2=points, K, radius) as called at PRE:56 / PRE:65:
 * first K points in index order with dist2 < radius^2 (fp32, no FMA).
 * idx (B,M,K) int32 pad -1; cluster (B,M,K,3) gathered xyz pad 0.0 (masked_gather,
 * PRE:627-672); pad_count (B,M) int32 = #(idx==-1) (PRE:372), may be NULL. */
PTX_API int ptx_ball_query(const float *centers, const float *points, int B, int M, int N, int K,
                   float radius, int32_t *idx, float *cluster, int32_t *pad_count, void *stream);

/* nn.Linear as used throughout ProxyAttention / Mlp (PRE:221, 223, 255; timm Mlp fc1/fc2):
 * y (rows,n_out) = x (rows,n_in) w^T (n_out,n_in) + bias [-> GELU(erf) if gelu] [+ residual].
 * fp32 MFMA (v_mfma_f32_32x32x2_f32); n_in % 4 == 0, x and w 16-byte aligned. */
PTX_API int ptx_linear(const float *x, const float *w, const float *bias, const float *residual, float *y,
               int rows, int n_out, int n_in, int gelu, void *stream);
/* The LayerNorm -> Linear seam of the eval forward (norm2 -> fc1 of both blocks, norm_img -> proxy_proj), as operators: the same
 * launch_gemm / k_prep_lnfold calls the forward makes, steered by ptx_gemm_policy the same way.
 * Producer: ptx_linear without GELU, and per row and per 32-column tile of y the fp32 LayerNorm partial of the FINAL values,
 * lnp[(row * ceil(n_out / 32) + tile) * 2 + {0, 1}] (rows * ceil(n_out / 32) * 2 floats, 8-byte aligned). */
PTX_API int ptx_linear_ln_partials(const float *x, const float *w, const float *bias, const float *residual, float *y, float *lnp,
               int rows, int n_out, int n_in, void *stream);
/* Consumer: y (rows,n_out) = Linear(LayerNorm(x; gamma, beta, eps); w, bias) [-> GELU(erf)] on the RAW rows x (rows,n_in) of a
 * producer and its partials lnp (rows, n_in / 32, 2); the normalised rows are never formed.  n_in a multiple of 32, at most 512
 * (anything else is PTX_EINVAL, nothing is launched); bias may be NULL.  scratch: ptx_ln_linear_scratch_bytes(n_out, n_in) bytes,
 * 16-byte aligned, overwritten with the folded tables (w diag(gamma), w beta + bias). */
PTX_API size_t ptx_ln_linear_scratch_bytes(int n_out, int n_in);
PTX_API int ptx_ln_linear(const float *x, const float *lnp, const float *w, const float *gamma, const float *beta,
               const float *bias, float eps, int gelu, float *y, void *scratch, size_t scratch_bytes,
               int rows, int n_out, int n_in, void *stream);
/* ABI 12.  Tile policy of the split-operand GEMMs behind every nn.Linear of the path (csrc/gemm.hip): a launch (all its groups
 * together) of at least `min_tiles_128` tiles of 128 x 128 outputs, with K a multiple of 256, runs on 128 x 128 tiles (k_gemm128x),
 * anything else on 64 x 64 tiles / the latency-regime kernel (between 1 and 1.5 x `min_tiles_128` tiles the large tile is taken only
 * for K >= 512).  Default 256 (one tile per CU); 0 = never; 1 = whenever the shape
 * allows it (tests); < 0 = query.  Returns the previous value.  Process-wide, relaxed: results do not depend on it beyond the
 * summation order of an fp32-equivalent product. */
PTX_API int ptx_gemm_policy(int min_tiles_128);

/* OffsetNetwork.forward + tanh*margin + add + clamp, PRE:58-62, 87-107.
 * centers_in (B,M,3), cluster (B,M,K,3), minmax (B,2,3) -> centers_out (B,M,3);
 * offsets_out (B,M,3) = tanh(raw)*margin, may be NULL. */
PTX_API int ptx_offset_net(const PtxShape *s, const PtxWeights *w, const void *prep,
                   const float *centers_in, const float *cluster, const float *minmax,
                   float *centers_out, float *offsets_out, void *stream);

/* dynamic_cluster_dropout, PRE:352-420, argsort tie-break pinned to stable ascending.
 * order_override (B,Mt) int32 or NULL: test-only replay of a captured argsort.
 * Outputs: order (B,Mt), picks (B,Kd) FPS positions, keep (B,Mk) positions,
 * kcenter (B,Mk,3), kcluster (B,Mk,K,3), kidx (B,Mk,K), drop_idx (B,Kd*K);
 * tag (B,N) uint32 (every word is written; since r05 the buffer need not be cleared): low 31 bits <- 1 + last (m,k) slot that owns the
 * point (pt_replace's last-writer rule, PRE:478-495), bit 31 <- point is dropped
 * (remove_points_by_index, PRE:516-523). */
PTX_API int ptx_select_clusters(const PtxShape *s, const int32_t *idx, const float *centers,
                        const float *cluster, const int32_t *pad_count,
                        const int32_t *order_override,
                        int32_t *order, int32_t *picks, int32_t *keep,
                        float *kcenter, float *kcluster, int32_t *kidx, int32_t *drop_idx,
                        uint32_t *tag, void *stream);

/* SimplifiedPointNet.forward, PRE:126-142 -> point_proxy (B,Mk,C). */
PTX_API int ptx_pointnet(const PtxShape *s, const PtxWeights *w, const void *prep, const float *kcenter,
                 const float *kcluster, float *point_proxy, void *stream);

/* get_img_proxy, PRE:335-342 (1x1 conv + AttentionPool2d token 0 + LayerNorm)
 * img_feat (B,V,in_dim,hw) of s->img_dtype -> img_proxy (B,V,C). */
PTX_API int ptx_img_proxy(const PtxShape *s, const PtxWeights *w, const void *prep, const void *img_feat,
                  float *img_proxy, void *workspace, size_t ws_bytes, void *stream);

/* ProxyBlock (eval) + trailing LayerNorm + Linear head + BatchNorm1d(eval):
 * which = 0: textformer[-1] -> translate (B,Mk,3)   PRE:441-446
 * which = 1: imgformer[-1]  -> transform (B,Mk,9)   PRE:450-455
 * proxy (B,Lp,C); mask (B,Lp) uint8 (1 = valid token) or NULL; guide (B,Mk,C) optional
 * copy of the normed block output (may be NULL). */
PTX_API int ptx_proxy_block(const PtxShape *s, const PtxWeights *w, const void *prep, int which,
                    const float *point_proxy, const float *proxy, int Lp, const uint8_t *mask,
                    float *head_out, float *guide, void *workspace, size_t ws_bytes, void *stream);

/* Per-cluster affine (PRE:459-462) + pt_replace (PRE:472-498) WITHOUT the drop:
 * new_points (B,N,3) = points with every owned point replaced by
 * T_j (p - c_j) + c_j + t_j, j = owning kept cluster (tag from ptx_select_clusters). */
PTX_API int ptx_affine_scatter(const PtxShape *s, const float *points, const uint32_t *tag,
                       const float *kcenter, const float *translate, const float *transform,
                       float *new_points, void *stream);

/* affine + pt_replace + remove_points_by_index (PRE:459-467, 501-525), order preserving.
 * out (B,N,3) capacity; counts (B) int32 = surviving points per scene (device). */
PTX_API int ptx_affine_compact(const PtxShape *s, const float *points, const uint32_t *tag,
                       const float *kcenter, const float *translate, const float *transform,
                       float *out, int32_t *counts, void *workspace, size_t ws_bytes, void *stream);

/* The two attention products of ProxyAttention (PRE:230-250) on projected inputs: qkv (B*n, 3C) rows [q | k | v] of the
 * cluster tokens (PRE:221), pt (B*Lp, C) = proxy_proj(proxy) (PRE:223), mask (B,Lp) uint8 (1 = valid; NULL: none),
 *   pv  = softmax_n((P scale) K^T) V                      (proxy as query, unmasked, PRE:232-238)
 *   out = softmax_L(masked_fill((Q scale) P^T, -1e9)) pv  (proxy as key, PRE:241-250), heads merged: out (B*n, C).
 * impl 0: the library's choice for the shape; 1: one fused launch (csrc/fattn.hip; head_dim 32 only); 2: two launches of
 * the fp32 matrix-instruction kernel (csrc/attn.hip), which need scratch for pv; 3: the fused launch with the proxies of
 * every (scene, head) in four slices on four work-groups, merged by the last to arrive (what the forward uses when a call
 * has few scenes), which needs scratch for tickets + partial results.  scratch: ptx_proxy_attention_scratch_bytes() bytes
 * for the impl passed (0 and 2: B*Lp*C floats). */
PTX_API size_t ptx_proxy_attention_scratch_bytes(int B, int n, int Lp, int heads, int C, int impl);
PTX_API int ptx_proxy_attention(const float *qkv, const float *pt, const uint8_t *mask, float *out, float *scratch, int B, int n,
                        int Lp, int heads, int C, int impl, void *stream);

/* Whole forward, PRE:424-469, enqueued on `stream` (the side streams of `ctx` fork the
 * clustering chain).  Points: either `points` (B,N,3) stacked, or `points_list` = HOST array of B
 * device pointers to (N,3) clouds (the reference's list input, used in place; B <= 32), the other
 * NULL.  text_mask (B,L) uint8, 1 = valid.  out (B,N,3) capacity, counts (B) int32 (device or
 * device-mapped pinned host memory).  counts is published with a system-scope store as soon as
 * the drop tags are final (well before the forward has drained): a caller that only needs the
 * output lengths on the host (PRE:467 returns a list of (N_i',3) views) presets counts[b] = -1
 * in pinned memory, calls ptx_forward and then ptx_wait_counts instead of synchronising the
 * stream; `out` itself is ordered on `stream` like any other asynchronous result.
 * debug (optional, may be NULL): struct of device pointers that receive intermediates. */
typedef struct PtxDebug {
    float *centers0, *cluster1, *offsets, *centers, *cluster2;
    int32_t *idx2, *pad_count, *order, *picks, *keep, *kidx, *drop_idx;
    float *kcenter, *kcluster, *point_proxy, *img_proxy, *text_guide, *img_guide;
    float *translate, *transform;
    uint32_t *tag;
} PtxDebug;

PTX_API int ptx_forward(PtxContext *ctx, const PtxShape *s, const PtxWeights *w, const void *prep, const float *lin,
                const float *points, const float *const *points_list, const float *text_feats,
                const uint8_t *text_mask, const void *img_feat, const int32_t *order_override,
                const float *centers_override,
                float *out, int32_t *counts, void *workspace, size_t ws_bytes,
                const PtxDebug *debug, void *stream);

/* ptx_forward with options (ABI 5).  opts = NULL is ptx_forward.
 *   bbox_enc       (B,6) uint32: the scenes' bounding boxes as ptx_ingest_gather publishes them (words 0..2 =
 *                  ~ord(min_xyz), 3..5 = ord(max_xyz), ord = the order-preserving float -> uint32 map); the forward then
 *                  skips its own min / max pass over the points (PRE:37-38).  Read-only here.
 *   compute_dtype  arithmetic of the ProxyBlock GEMMs and attention: 0 = fp32-equivalent (the parity path, default),
 *                  1 = plain bf16 operands with fp32 accumulation (throughput mode; the reference under --amp,
 *                  tools/train.py:93-105).  Index tensors are unaffected (the clustering half stays fp32). */
typedef struct PtxForwardOpts {
    const uint32_t *bbox_enc;
    int32_t compute_dtype;
    int32_t reserved[5];
} PtxForwardOpts;
PTX_API int ptx_forward_ex(PtxContext *ctx, const PtxShape *s, const PtxWeights *w, const void *prep, const float *lin,
                   const float *points, const float *const *points_list, const float *text_feats,
                   const uint8_t *text_mask, const void *img_feat, const int32_t *order_override,
                   const float *centers_override,
                   float *out, int32_t *counts, void *workspace, size_t ws_bytes,
                   const PtxDebug *debug, const PtxForwardOpts *opts, void *stream);

/* Host-side spin until counts_host[0..B) (pinned host memory, preset to -1 by the caller) are all
 * >= 0, or timeout_us elapses.  Returns 0 when the counts are there, PTX_ETIMEOUT otherwise
 * (the caller then falls back to a stream synchronise, which also surfaces device faults). */
PTX_API int ptx_wait_counts(const int32_t *counts_host, int B, int64_t timeout_us);

/* ------------------------------------------------------------------ multi-view depth ingest
 * What the reference's data pipeline computes on the host between the decoded depth maps and the (N,3) cloud handed to
 * the path (configs/grounding/proxy-tiblock33-gs12-wbias-ddr0.6-clip.py:105-142):
 *   ConvertRGBDToPoints       datasets/transforms/points.py:20-98  (points_img2cam, structures/bbox_3d/utils.py:336-368)
 *   PointSample per view      datasets/transforms/points.py:290-420          [np.random.choice on the host, or ptx_ingest_draw]
 *   AggregateMultiViewPoints  datasets/transforms/multiview.py:195-253       (torch.linalg.solve(global2ego, [p;1]))
 *   PointSample of the scene  datasets/transforms/points.py:290-420          [np.random.choice on the host, or ptx_ingest_draw]
 *   GlobalRotScaleTrans       datasets/transforms/augmentation.py:253-       (points only; parameters from the host)
 * depth (V,H,W): float32 metres (depth_dtype 0) or the decoded uint16 image (1; value / depth_shift as LoadDepthFromFile
 * does).  ptx_ingest_index builds a rank / select index over the pixels with depth != 0 (one streaming pass) and
 * publishes view_counts[v] = their number per view with system scope (device or pinned host int32: the host needs them
 * for `replace` of np.random.choice).  ptx_ingest_gather computes ONLY the N selected points: sel[j] (int64) = rank of
 * output point j in the concatenation over the views of each view's depth != 0 pixels in row-major order (the
 * reference's grid3d[nonzero_indices]; the host composes its two np.random.choice draws into it).
 * inv_intrinsic (V,4,4) = inverse of the 4x4-padded depth_cam2img; lu (V,4,4) + piv (V,4) int32 = LU factors of
 * global2ego with rows permuted by piv (P A = L U, unit lower); aug = NULL or 13 floats rot_mat_T (3,3) | scale | trans;
 * points (N,3); bbox_enc (6) uint32 or NULL = the cloud's bounding box in ptx_forward_ex's encoding (cleared here);
 * status (1) int32 device: bit 0 set if any sel[j] was out of range (that point is written as 0). */
PTX_API size_t ptx_ingest_workspace_bytes(int V, int H, int W);
PTX_API int ptx_ingest_index(const void *depth, int depth_dtype, int V, int H, int W, void *workspace, size_t ws_bytes,
                     int32_t *view_counts, void *stream);
PTX_API int ptx_ingest_gather(const void *depth, int depth_dtype, float depth_shift, int V, int H, int W, const float *inv_intrinsic,
                      const float *lu, const int32_t *piv, const int64_t *sel, int N, const float *aug, float *points,
                      uint32_t *bbox_enc, int32_t *status, const void *workspace, size_t ws_bytes, void *stream);

/* ABI 13.  The two PointSample draws ON THE DEVICE (MultiViewIngest(sampler="device"); the numpy path above stays the default and
 * the parity mode).  Runs on `stream` after ptx_ingest_index, reads the per-view counts from the index workspace and writes
 * sel (N int64, device) for the unchanged ptx_ingest_gather: the host neither waits for the counts nor uploads anything per point.
 * The draws are a pure function of (key, view counts, per_view, N) -- integer arithmetic only, the same on every device and stream --
 * and follow the reference's rules (points.py:335-336, 395-411; multiview.py:195-253); they do not reproduce numpy's stream.
 * ingest.device_choices restates them exactly on the host.  Definition (all arithmetic mod 2^64):
 *   mix(z)      splitmix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   G           0x9E3779B97F4A7C15
 *   K(s)        stage key = mix(key ^ mix(s + G)):  s = 0 the aggregate draw, s = v + 1 the draw of view v
 *   P(k, m, x)  keyed permutation of [0, m): h = max(1, ceil(bitlen(m - 1) / 2)); a balanced Feistel network on 2h bits,
 *               (L, R) = (x >> h, x & (2^h - 1)), 6 rounds r = 0..5 of (L, R) <- (R, L ^ (mix(k ^ ((r + 1) << 56) ^ R) >> (64 - h))),
 *               x <- (L << h) | R; repeated (cycle walking) until x < m.  A draw without replacement of n out of m is P(k, m, 0..n-1):
 *               distinct, in random order (never sorted), as np.random.choice(m, n, replace=False) returns them.
 *   U(k, m, i)  draw with replacement: the high 64 bits of mix(k + (i + 1) * G) * m (every value within 2^-64 of probability 1/m)
 *   cnt_v       depth != 0 pixels of view v, off_v = those of the views before v; E = views with cnt_v > 0, T = E * per_view
 *   per output point j in [0, N):  q = T >= N ? P(K(0), T, j) : U(K(0), T, j);  e = q / per_view, i = q % per_view;
 *               v = the e-th view with cnt_v > 0 (view order);  sel[j] = off_v + (cnt_v >= per_view ? P(K(v+1), cnt_v, i)
 *                                                                                                   : U(K(v+1), cnt_v, i))
 * status (1 int32, device): written by the kernel, PTX_DRAW_EMPTY when no view has a pixel (E = 0; sel is then all zeros, which
 * ptx_ingest_gather reports in its own status word), 0 otherwise.  Host checks only (PTX_EINVAL before anything is enqueued):
 * null pointers, V, H, W, per_view, N >= 1, V <= PTX_DRAW_MAX_VIEWS. */
#define PTX_DRAW_EMPTY 1
#define PTX_DRAW_MAX_VIEWS 4096
PTX_API int ptx_ingest_draw(int V, int H, int W, int per_view, int N, uint64_t key, const void *workspace, size_t ws_bytes,
                    int64_t *sel, int32_t *status, void *stream);

/* ------------------------------------------------------------------ voxel quantisation
 * The step right after the path in the reference's detector (detectors/sparse_featfusion_grounder_preshape.py:388-397):
 * ME.utils.batch_sparse_collate([(p[:, :3] / voxel_size, p) ...]) + ME.SparseTensor(coordinates, features), i.e.
 * coordinates (b, floor(p / voxel_size)) int32 and ONE row per occupied voxel.  MinkowskiEngine is not vendored: the
 * surviving duplicate / row order are pinned to the first point of every voxel in (scene, point) order.
 * points (B,Ncap,3) with counts[b] valid rows per scene (device int32) = exactly the `out` / `counts` of ptx_forward;
 * coords (B*Ncap,4) int32 and feats (B*Ncap,3) capacity; inverse (B,Ncap) int32 voxel row of every point (-1 past the
 * valid rows) or NULL; nvox_overflow: 2 int32 = {voxel rows written, points whose voxel index left +-2^18}, device memory or
 * device-mapped pinned host memory: published with system scope as soon as the count is KNOWN (preset to -1 and poll with
 * ptx_wait_counts instead of draining the stream); the rows themselves are ordered on `stream` like any other result.
 * Rows written == PTX_VOX_BROKEN (0x7fffffff): a tile of the single-pass emit gave up waiting for the tiles in front of it
 * (2^24 polls); rows, inverse and the count of that call are invalid.
 * The key range: a voxel index is kept when it lies in [-2^18, 2^18) on every axis (scene < 64).  A point with a NaN or infinite
 * coordinate has no voxel: it is OUTSIDE the range and is counted in nvox_overflow[1] like a coordinate past +-2^18 (a NaN quotient
 * would convert to the integer 0; the range test therefore asks for a finite quotient first). */
#define PTX_VOX_BROKEN 0x7fffffff
PTX_API size_t ptx_voxel_workspace_bytes(int B, int Ncap);
PTX_API int ptx_voxelize(const float *points, const int32_t *counts, int B, int Ncap, float voxel_size, int32_t *coords,
                 float *feats, int32_t *inverse, int32_t *nvox_overflow, void *workspace, size_t ws_bytes, void *stream);
/* ABI 12.  ptx_voxelize + `scene_end` (B int32, device memory or device-mapped pinned host memory preset to -1; NULL = ptx_voxelize):
 * scene_end[b] = rows written for scenes 0..b, published with system scope by the last tile of scene b -- what a caller needs to
 * split the rows per scene (ME's decomposed_coordinates, DET:391-392, 429-430) without reading the scene column back. */
PTX_API int ptx_voxelize_ex(const float *points, const int32_t *counts, int B, int Ncap, float voxel_size, int32_t *coords,
                    float *feats, int32_t *inverse, int32_t *nvox_overflow, int32_t *scene_end, void *workspace, size_t ws_bytes,
                    void *stream);
/* ABI 13, by addition.  ptx_voxelize_ex + `rep` (B*Ncap int32 capacity; NULL = ptx_voxelize_ex): rep[r] = the flat padded index
 * b * Ncap + i of the point whose coordinates are feats[r] -- `features = p[unique_index]` of the quantisation (DET:388-397 with
 * use_xyz_feat, CFG:43), i.e. the index autograd hands row r's gradient back to.  One more store per row in the emit pass; coords,
 * feats, inverse, scene_end and the published counts are bit-identical to ptx_voxelize_ex on the same input. */
PTX_API int ptx_voxelize_rep(const float *points, const int32_t *counts, int B, int Ncap, float voxel_size, int32_t *coords,
                     float *feats, int32_t *inverse, int32_t *rep, int32_t *nvox_overflow, int32_t *scene_end, void *workspace,
                     size_t ws_bytes, void *stream);
/* ABI 13, by addition.  The backward of the features of DET:388-397 (`features = p[unique_index]`, a gather of whole rows) with
 * respect to the points: dfeats (nvox,3) fp32; inverse (B,Ncap), rep and counts (B, device) as ptx_voxelize_rep wrote / read them;
 * dpoints (B,Ncap,3) fp32.  Point (b,i), i < counts[b], receives dfeats[inverse[b,i]] if rep[inverse[b,i]] == b * Ncap + i and exact
 * zeros otherwise (the other points of a voxel).  One per-point pass on `stream`: every element of dpoints below the counts is
 * written exactly once, zeros included (rows past a count: when Ncap is a multiple of 4 and inverse / dpoints are 16-byte aligned,
 * the rest of the group of four points in which a scene's count ends is written as +0.0; nothing else past a count is touched) --
 * no memset, no float atomics, no workspace, no host wait, bitwise reproducible.  The coordinates (floor) get no gradient.  dfeats may be NULL when nvox == 0. */
PTX_API int ptx_voxel_features_bwd(const float *dfeats, int nvox, const int32_t *inverse, const int32_t *rep, const int32_t *counts,
                           int B, int Ncap, float *dpoints, void *stream);
/* ABI 12.  The coordinates of a COARSER MinkowskiEngine level over voxel rows the calls above produced -- what a strided layer of the
 * detector's sparse backbone does to its coordinate map (backbones/mink_resnet.py:57-78: tensor strides 8 / 16 / 32 / 64), which is all
 * the image-feature sampling behind it needs of that backbone (DET:429-430 `x[level].decomposed_coordinates[idx] * voxel_size`):
 * coords_in (rows,4) int32 (scene, x, y, z), scene b's rows [in_scene_end[b-1], in_scene_end[b]) with in_scene_end a [host] array
 * of B ints (read during the call); every row maps to floor(c / stride) * stride (stride: a power of two), one output row per
 * distinct result in first-occurrence order: coords (rows,4) int32 and points (rows,3) fp32 = coordinate * voxel_size.
 * nvox_overflow / scene_end / workspace as ptx_voxelize_ex (workspace: ptx_voxel_workspace_bytes(B, largest scene's rows)).  The key
 * range applies to the COARSE index: a row is kept when floor(c / stride) lies in [-2^18, 2^18) on every axis, i.e. c in
 * [-2^18 * stride, 2^18 * stride); any other row is counted in nvox_overflow[1]. */
PTX_API int ptx_voxel_coarsen(const int32_t *coords_in, const int32_t *in_scene_end, int B, int stride, float voxel_size,
                      int32_t *coords, float *points, int32_t *nvox_overflow, int32_t *scene_end, void *workspace, size_t ws_bytes,
                      void *stream);

/* ------------------------------------------------------------------ sparse 3D convolution on the voxel rows (ABI 13, by addition)
 * The primitive of `x = self.backbone_3d(x)` (DET:398; backbones/mink_resnet.py:58-63 conv1 = MinkowskiConvolution(3, 64, kernel_size=3,
 * stride=2), mink_resnet.py:67-69 MinkowskiMaxPooling(kernel_size=2, stride=2), mink_resnet.py:103-109 the 1x1 stride-2 downsample,
 * mink_resnet.py:111-119 the BasicBlocks' 3x3x3 convolutions): kernel maps over the rows the calls above produce, and a fused gather-GEMM convolution and max-pool that consume
 * them, and their backward passes.  MinkowskiInstanceNorm (mink_resnet.py:64) and a training MinkowskiBatchNorm: the norm section below; the backbone is
 * assembled in Python (proxytransformation_amd/backbone.py); neck_3d: the sparse-neck section below.
 *
 * Kernel map.  coords_in (n_in,4) int32 rows (scene, x, y, z) of a level of tensor stride `tensor_stride` (a power of two; every
 * coordinate a multiple of it), scene b's rows [in_scene_end[b-1], in_scene_end[b]) with in_scene_end a [host] array of B ints (read
 * during the call).  Output rows: stride 1 -- the input rows (coords_out is not written and may be NULL); stride 2 -- the distinct
 * floor(c / (2 tensor_stride)) * (2 tensor_stride) per scene in first-occurrence order, written to coords_out (n_in rows capacity) by
 * ptx_voxel_coarsen itself (same rows, same order).  Offsets: odd kernel_size {-(k/2) .. k/2} * tensor_stride per axis around the output
 * coordinate, even kernel_size {0 .. k-1} * tensor_stride; never across scenes; offset index j = (dz * k + dy) * k + dx counted from the
 * lowest offset, x fastest (MinkowskiEngine's region iterator as we read it: parity unpinned against ME itself).  nbr (n_in * k^3 int32
 * capacity): nbr[o * k^3 + j] = the input row at (output row o's coordinate + offset j), or -1.
 * count_words: 2 int32 = {output rows, rows whose coordinate >> log2(stride of the table) left +-2^18}; out_scene_end: B int32 ends of
 * the output rows per scene; both device memory or device-mapped pinned host memory preset to -1, published with system scope (poll
 * with ptx_wait_counts; no device synchronise); rows == PTX_VOX_BROKEN as for ptx_voxelize.  The rows and nbr are ordered on `stream`.
 * workspace: ptx_sparse_kernel_map_workspace_bytes(B, ncap >= the largest scene's rows) bytes, 256-byte aligned (two hash tables of
 * ptx_voxel_workspace_bytes each: the coarsening's and the index of the input rows, whose value is the row).  B <= 64.  Host checks
 * (PTX_EINVAL / PTX_ENOSPACE with a message) come before anything is enqueued. */
PTX_API size_t ptx_sparse_kernel_map_workspace_bytes(int B, int ncap);
PTX_API int ptx_sparse_kernel_map(const int32_t *coords_in, const int32_t *in_scene_end, int B, int tensor_stride, int kernel_size, int stride,
                          int32_t *coords_out, int32_t *out_scene_end, int32_t *nbr, int32_t *count_words, void *workspace,
                          size_t ws_bytes, void *stream);
/* out (n_out,Cout) fp32:  out[o] = sum_j feats[nbr[o * kvol + j]] @ weight[j]  over the neighbours that are present (a row without any
 * is zero), then, each part optional (NULL / 0):  + bias[c];  * scale[c] + shift[c] (an eval MinkowskiBatchNorm folded by the caller,
 * mink_resnet.py:109);  + residual[o,c];  ReLU.  feats (n_in,Cin) fp32, weight (kvol,Cin,Cout) fp32 -- the layout of
 * ME.MinkowskiConvolution's `kernel` parameter --, bias / scale / shift (Cout), residual (n_out,Cout); kvol 1, 8 or 27.  One launch of
 * 64-row x 64-channel tiles on the exact-fp32 matrix instruction; blocked summation (per offset and 64 input channels, then over those
 * blocks) in a fixed order, no float atomics: bitwise reproducible.
 * Cout: a multiple of 64 up to 512; Cin: a multiple of 16 up to 512, or 3 with kvol 27 (the stem, mink_resnet.py:58-63: one K = 81
 * panel).  Anything else is PTX_EINVAL with the numbers in the message, before anything is enqueued.  `out` must not alias feats. */
PTX_API int ptx_sparse_conv3d(const float *feats, int n_in, const int32_t *nbr, int n_out, int kvol, const float *weight, int Cin, int Cout,
                      const float *bias, const float *scale, const float *shift, const float *residual, int relu, float *out,
                      void *stream);
/* out (n_out,C) fp32 = max over the present neighbours of feats[nbr[o * kvol + j]] (MinkowskiMaxPooling, mink_resnet.py:67-69; with
 * kernel_size 2, stride 2 every output row has one; a row without any is -inf).  C: a multiple of 4.  nbr must come from
 * ptx_sparse_kernel_map over feats' rows (indices are not range-checked). */
PTX_API int ptx_sparse_max_pool3d(const float *feats, const int32_t *nbr, int n_out, int kvol, int C, float *out, void *stream);
/* Backward of the two layers (ABI 13, by addition) -- the coordinate manager run backwards.  No float atomics: every output is bitwise
 * reproducible launch to launch; everything is ordered on `stream`, no host wait; host checks come before anything is enqueued.
 *
 * Transposed map: nbr_t (n_in,kvol) int32, nbr_t[i * kvol + j] = the output row o with nbr[o * kvol + j] == i, else -1 (for a fixed (i, j)
 * at most one exists: its coordinate is coord_i - offset_j).  Entries of nbr < 0 or >= n_in are skipped.  One fill + one launch. */
PTX_API int ptx_sparse_kernel_map_transpose(const int32_t *nbr, int n_out, int kvol, int n_in, int32_t *nbr_t, void *stream);
/* Gradients of ptx_sparse_conv3d, given g = d loss / d out (n_out,Cout).  With out the forward's result (read only when relu) and
 * gz = g * [out > 0] * scale (either factor only when present):
 *   dresidual (n_out,Cout) = g * [out > 0];   dbias (Cout) = sum_o gz[o] (256-row tiles, then the tiles, both in a fixed blocked order);
 *   dfeats (n_in,Cin): dfeats[i] = sum_j gz[nbr_t[i * kvol + j]] @ weight[j]^T  (the forward kernel over the transposed map);
 *   dweight (kvol,Cin,Cout): dweight[j] = sum_o feats[nbr[o * kvol + j]]^T @ gz[o], split over row chunks: 64-pair steps on the exact-fp32
 *   matrix instruction, each from zero and added to the chunk's running sum, the chunks' partials added in ascending order.
 * Each of dresidual / dbias / dfeats / dweight is optional (NULL: not computed, and its work is not done).  gz (n_out,Cout) is scratch
 * the call writes; it is needed when (relu or scale) and (dfeats or dweight).  scale / shift get no gradient (a folded frozen BatchNorm).
 * Cout: a multiple of 64 up to 512; Cin: a multiple of 64 up to 1024 (the neck's out_block_3 is 27 x 1024 -> 256), or 3 with kvol 27
 * (the stem); kvol 1, 8 or 27; anything else is PTX_EINVAL with the numbers.  workspace: ptx_sparse_conv3d_bwd_workspace_bytes(n_out, kvol, Cin, Cout) bytes (0: unsupported), 16-byte
 * aligned; needed for dbias and dweight.  All float buffers 16-byte aligned; the outputs must not alias the inputs. */
PTX_API size_t ptx_sparse_conv3d_bwd_workspace_bytes(int n_out, int kvol, int Cin, int Cout);
PTX_API int ptx_sparse_conv3d_bwd(const float *g, const float *out, const float *scale, int relu, const float *feats, int n_in,
                          const int32_t *nbr, const int32_t *nbr_t, int n_out, int kvol, const float *weight, int Cin, int Cout,
                          float *gz, float *dresidual, float *dbias, float *dfeats, float *dweight, void *workspace, size_t ws_bytes,
                          void *stream);
/* ptx_sparse_max_pool3d plus arg (n_out,C) uint8: the offset index j that supplied the maximum, 255 for a row without neighbours.  Ties
 * go to the smallest j.  `out` is bit-identical to ptx_sparse_max_pool3d's. */
PTX_API int ptx_sparse_max_pool3d_arg(const float *feats, const int32_t *nbr, int n_out, int kvol, int C, float *out, uint8_t *arg,
                              void *stream);
/* dfeats (n_in,C): dfeats[i,c] = sum over ascending j of [arg[nbr_t[i * kvol + j], c] == j] * g[nbr_t[i * kvol + j], c]; every element
 * is written once. */
PTX_API int ptx_sparse_max_pool3d_bwd(const float *g, const uint8_t *arg, const int32_t *nbr_t, int n_in, int n_out, int kvol, int C,
                              float *dfeats, void *stream);

/* ------------------------------------------------------------------ instance norm / training batch norm on the voxel rows (ABI 13, by addition)
 * MinkowskiInstanceNorm (mink_resnet.py:67: per scene) and a training MinkowskiBatchNorm (one segment over all rows) are the same
 * kernels: column moments per row segment -> normalise -> affine (+ residual)(+ ReLU), forward and backward.  x (n,C) fp32, C a multiple
 * of 64 up to 512; seg_end: a [host] array of S ints, 1 <= S <= 64, the ascending ends of the segments' rows with seg_end[S-1] == n
 * (ptx_sparse_kernel_map's in_scene_end; read during the call; empty segments allowed).  Tiles of 256 rows that never straddle a
 * segment; per tile (mean, M2 about that mean), merged per segment with Chan's formula in a fixed blocked ascending order -- never
 * E[x^2] - E[x]^2; no float atomics: two calls on the same inputs give the same bits.  Everything is ordered on `stream`, no host wait;
 * the checks (PTX_EINVAL / PTX_ENOSPACE with a message) come before anything is enqueued.  All float buffers and the workspace
 * (ptx_sparse_norm_workspace_bytes(n, S, C) bytes; 0: unsupported size) 16-byte aligned.
 *
 * Forward: stats (S,2,C) = per segment and column (mean, rstd = 1 / sqrt(var_biased + eps)), an empty segment (0, 0);
 * out = relu?(((x - mean) * rstd) * weight + bias (+ residual)), weight / bias (C), residual (n,C), each optional (NULL).  A one-row
 * segment has variance 0: its output is bias (+ residual).  running_mean / running_var (C), both or neither, only with S == 1 and
 * n >= 2: updated in place, (1 - momentum) * old + momentum * new with the unbiased variance M2 / (n - 1) (nn.BatchNorm1d's rule). */
PTX_API size_t ptx_sparse_norm_workspace_bytes(int n, int S, int C);
PTX_API int ptx_sparse_norm_fwd(const float *x, const int32_t *seg_end, int S, int n, int C, float eps, const float *weight,
                        const float *bias, const float *residual, int relu, float *running_mean, float *running_var, float momentum,
                        float *stats, float *out, void *workspace, size_t ws_bytes, void *stream);
/* The forward's last pass alone, from stats the caller supplies (an eval batch norm: mean = running_mean, rstd from running_var). */
PTX_API int ptx_sparse_norm_apply(const float *x, const int32_t *seg_end, int S, int n, int C, const float *stats, const float *weight,
                          const float *bias, const float *residual, int relu, float *out, void *stream);
/* Backward, given g = d loss / d out (n,C), x and the forward's stats; out: the forward's result when it had a ReLU, else NULL.
 * gy = g * [out > 0] (g itself without ReLU); xhat = (x - mean) * rstd recomputed;  dresidual (n,C) = gy;  dbias (C) = sum_rows gy;
 * dweight (C) = sum_rows gy * xhat;  per segment a = mean_s(gy), b = mean_s(gy * xhat);  dx = weight * rstd_s * ((gy - a) - xhat * b).
 * Every output pointer is optional (NULL: not computed).  The workspace is always needed. */
PTX_API int ptx_sparse_norm_bwd(const float *g, const float *x, const float *out, const int32_t *seg_end, int S, int n, int C,
                        const float *stats, const float *weight, float *dx, float *dweight, float *dbias, float *dresidual,
                        void *workspace, size_t ws_bytes, void *stream);
/* The same forward and backward with an activation selector in the place of the ReLU flag (ABI 13, by addition; the neck's training
 * BatchNorms, mink_neck.py:96-104: MinkowskiBatchNorm + MinkowskiELU): act 0 none, 1 ReLU, 2 ELU with alpha = 1, v > 0 ? v : expm1f(v).
 * Selectors 0 and 1 give ptx_sparse_norm_fwd's / ptx_sparse_norm_bwd's bits.  Backward: out is the forward's result (needed unless
 * act == 0); behind an ELU gy = g * (out > 0 ? 1 : out + 1) from the saved out -- exactly 0 where out == -1.  THE NaN RULE: a NaN in
 * out gives a NaN gy (NaN > 0 is false and g * (NaN + 1) is NaN): it is never dropped, unlike behind a ReLU, where [NaN > 0] = 0. */
PTX_API int ptx_sparse_norm_fwd_act(const float *x, const int32_t *seg_end, int S, int n, int C, float eps, const float *weight,
                            const float *bias, const float *residual, int act, float *running_mean, float *running_var, float momentum,
                            float *stats, float *out, void *workspace, size_t ws_bytes, void *stream);
PTX_API int ptx_sparse_norm_bwd_act(const float *g, const float *x, const float *out, int act, const int32_t *seg_end, int S, int n, int C,
                            const float *stats, const float *weight, float *dx, float *dweight, float *dbias, float *dresidual,
                            void *workspace, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ the sparse neck: MinkNeck, eval forward (ABI 13, by addition)
 * `feats, scores, coords = self.neck_3d(x, batch_size)` (necks/mink_neck.py:142-161): the generative transposed convolution, the sum
 * over the union of two row sets, the trilinear score lookup, the per-scene top-k prune and the classification head, plus the
 * convolution with an activation selector and wide inputs.  The neck is assembled in Python (proxytransformation_amd/neck.py) and
 * restated in numpy (neck_host.py).  fp32; no float atomics and fixed summation orders: two calls on the same inputs give the same bits;
 * everything is ordered on `stream`; the host waits only for the union's row counts (pinned words, ptx_wait_counts) and never
 * synchronises the device; host checks (PTX_EINVAL / PTX_ENOSPACE with the numbers in the message) come before anything is enqueued.
 * Rows, scene ends ([host] arrays of B ints, B <= 64) and tensor strides are ptx_sparse_kernel_map's.  These are the forward's entry
 * points; the backward and the training BatchNorm are the next section's.  No bf16.
 *
 * ptx_sparse_conv3d with `act` a selector -- 0 none, 1 ReLU (ptx_sparse_conv3d's bits), 2 ELU alpha = 1: v > 0 ? v : expm1f(v) -- and
 * Cin a multiple of 16 up to 1024 (or the stem's 3).  The same kernel. */
PTX_API int ptx_sparse_conv3d_act(const float *feats, int n_in, const int32_t *nbr, int n_out, int kvol, const float *weight, int Cin, int Cout,
                          const float *bias, const float *scale, const float *shift, const float *residual, int act, float *out,
                          void *stream);
/* MinkowskiGenerativeConvolutionTranspose(kernel_size=2, stride=2) (mink_neck.py:90-94): coords (n,4) of tensor stride
 * `tensor_stride` >= 2, feats (n,Cin), weight (8,Cin,Cout).  Row 8 i + j of coords_out (8 n,4) is coords[i] + offset j of a kernel of 2 at
 * tensor_stride / 2 (j counts x fastest, then y, then z: our reading of MinkowskiEngine, parity unpinned against ME itself), row 8 i + j of
 * out (8 n,Cout) is act(feats[i] @ weight[j] (* scale + shift)): the dense product (n,Cin) @ (Cin, 8 Cout) on the exact-fp32 matrix
 * instruction in ptx_sparse_conv3d's blocked order.  Children of distinct parents are distinct: no table.  Scene ends: 8 x the input's.
 * Cin: a multiple of 64 up to 1024; Cout: a multiple of 64 up to 512; act as above.  Two launches. */
PTX_API int ptx_sparse_conv_transpose_gen(const int32_t *coords, int n, int tensor_stride, const float *feats, const float *weight, int Cin,
                                  int Cout, const float *scale, const float *shift, int act, int32_t *coords_out, float *out, void *stream);
/* Workspace of the three calls below: B scenes, ncap >= the largest scene's rows of the set that is indexed (A's, the score rows'),
 * rows >= the rows of either operand of the union (0 for the score lookup).  0: unsupported size. */
PTX_API size_t ptx_neck_workspace_bytes(int B, int ncap, int rows);
/* `inputs[i] + x` (mink_neck.py:149): A and B, rows of the same tensor stride and width C (a multiple of 4), both grouped by scene.  The
 * result's rows of scene b are A's rows of b in A's order, then the rows of B in b that are absent from A, in B's order; features
 * A[a] + B[k] where both exist (one fp32 add), the single operand's row elsewhere.  B's rows must be distinct.  out_coords / out_feats:
 * capacity rows(A) + rows(B).  count_words: 2 int32 = {rows, rows of A whose coordinate >> log2(tensor_stride) left +-2^18};
 * out_scene_end: B int32; published like ptx_sparse_kernel_map's (preset to -1, poll with ptx_wait_counts).  The lookup of B's
 * coordinates in A is the kernel maps' hash table.  One memset pair + four launches. */
PTX_API int ptx_neck_union_add(const int32_t *a_coords, const int32_t *a_scene_end, const float *a_feats, const int32_t *b_coords,
                       const int32_t *b_scene_end, const float *b_feats, int B, int tensor_stride, int C, int32_t *out_coords,
                       float *out_feats, int32_t *out_scene_end, int32_t *count_words, void *workspace, size_t ws_bytes, void *stream);
/* `scores.features_at_coordinates(x.C.float())` (mink_neck.py:175): scores (m,1) on the rows s_coords of tensor stride ts =
 * `tensor_stride`, q_coords (n_q,4) any integer coordinates (the neck's are multiples of ts / 2).  Per axis l = floor(q / ts) * ts; the
 * eight corners c = l + {0, ts}^3, indexed x fastest; w_c = prod_axis (1 - |q - c| / ts); out[i] = sum over the corners present in the
 * same scene of w_c * scores[c], in ascending corner index from 0.0f (absent corners contribute nothing, nothing is renormalised, a
 * query without a present corner gets 0.0).  Bit-identical to the fp32 numpy restatement. */
PTX_API int ptx_neck_prune_scores(const int32_t *q_coords, int n_q, const int32_t *s_coords, const int32_t *s_scene_end, int B,
                          int tensor_stride, const float *scores, float *out, void *workspace, size_t ws_bytes, void *stream);
/* The per-scene top-k of mink_neck.py:178-185 with MinkowskiPruning: scene b keeps its min(rows_b, k) rows with the largest scores (n);
 * among equal scores the lower row index wins (torch.topk leaves ties unspecified); -0.0 and +0.0 are equal; a NaN orders by its bits
 * (above +inf with the sign bit clear, below -inf with it set).  dest (n) int32: the place of each row among the kept rows, or -1; the
 * kept rows keep their relative order; coords (n,4) / feats (n,C) are copied to out_coords / out_feats at dest.  The new scene ends are
 * the accumulated min(rows_b, k): the host knows them without a wait.  A radix select per scene, integer counts only.  Two launches. */
PTX_API int ptx_neck_topk_prune(const float *scores, const int32_t *scene_end, int B, int k, const int32_t *coords, const float *feats, int C,
                        int32_t *dest, int32_t *out_coords, float *out_feats, void *stream);
/* conv_cls (kernel 1, with bias; mink_neck.py:122-126) and the prune score of mink_neck.py:200-201 in one kernel: cls (n,num_classes) =
 * feats (n,C) @ weight (C,num_classes) + bias (num_classes, optional), score (n) = max over the classes of cls.  C: a multiple of 64 up
 * to 512; 1 <= num_classes <= 16.  Fixed order: 16 lanes per row, each its channels 4 l + 64 m ascending, then the lanes by halving. */
PTX_API int ptx_neck_head(const float *feats, int n, int C, const float *weight, const float *bias, int num_classes, float *cls, float *score,
                  void *stream);

/* ------------------------------------------------------------------ the sparse neck in training mode: the backward (ABI 13, by addition)
 * The reference trains the neck with its BatchNorms in training mode and prunes under torch.no_grad() (necks/mink_neck.py:163-186):
 * features and cls_preds carry gradient; the prune scores, the trilinear lookup and the top-k do not.  The chain (mink_neck.py:142-161)
 * is assembled in Python (neck.MinkNeck(differentiable=True)): every block is a raw convolution followed by ptx_sparse_norm_fwd_act with
 * the ELU; the convolutions' backward is ptx_sparse_conv3d_bwd.  fp32, no float atomics, fixed summation orders: two calls on the same
 * inputs give the same bits; everything on `stream`, no host wait; host checks (PTX_EINVAL / PTX_ENOSPACE with the numbers) come first.
 *
 * Backward of ptx_sparse_conv_transpose_gen without its epilogue (mink_neck.py:90-94; the BatchNorm is separate), g (8 n,Cout):
 *   dfeats (n,Cin): dfeats[i] = sum_j g[8 i + j] @ weight[j]^T -- the dense (n, 8 Cout) @ (8 Cout, Cin) product, no table;
 *   dweight (8,Cin,Cout): dweight[j] = feats^T @ g[j::8], split over row chunks into slabs added in ascending order
 * on the exact-fp32 matrix instruction, in ptx_sparse_conv3d_bwd's kernels and order.  Each output is optional (NULL).  Cin: a multiple
 * of 64 up to 1024; Cout: a multiple of 64 up to 512; n <= 2^24.  workspace: ptx_sparse_conv_transpose_gen_bwd_workspace_bytes(n, Cin,
 * Cout) bytes, a function of the shapes only (0: unsupported), needed for dweight. */
PTX_API size_t ptx_sparse_conv_transpose_gen_bwd_workspace_bytes(int n, int Cin, int Cout);
PTX_API int ptx_sparse_conv_transpose_gen_bwd(const float *g, const float *feats, int n, const float *weight, int Cin, int Cout, float *dfeats,
                                      float *dweight, void *workspace, size_t ws_bytes, void *stream);
/* ptx_neck_union_add (mink_neck.py:149) that also records where every input row went: a_dest (nA) / b_dest (nB) int32 = the row of the
 * result that holds A[a] resp. B[k] (a matched pair shares one), -1 for a row outside every scene.  Same results, bit for bit. */
PTX_API int ptx_neck_union_add_dest(const int32_t *a_coords, const int32_t *a_scene_end, const float *a_feats, const int32_t *b_coords,
                            const int32_t *b_scene_end, const float *b_feats, int B, int tensor_stride, int C, int32_t *out_coords,
                            float *out_feats, int32_t *out_scene_end, int32_t *count_words, int32_t *a_dest, int32_t *b_dest, void *workspace,
                            size_t ws_bytes, void *stream);
/* out (n,C): out[i] = 0 <= dest[i] < n_src ? g[dest[i]] : +0.0 with g (n_src,C), C a multiple of 4; 16-byte accesses, pure copies.  The
 * backward of the three row routings: dA = g[a_dest], dB = g[b_dest] of the union, and dU of MinkowskiPruning (mink_neck.py:186) from the
 * dest ptx_neck_topk_prune writes (dropped rows get +0.0).  n == 0: no launch. */
PTX_API int ptx_neck_rows_gather(const float *g, int n_src, const int32_t *dest, int n, int C, float *out, void *stream);
/* Backward of conv_cls in ptx_neck_head (mink_neck.py:122-126, 200), given dcls (n,num_classes); the prune score is detached (the
 * reference takes it under no_grad).  dfeats (n,C) = dcls @ weight^T, the classes added in ascending order; dweight (C,num_classes) =
 * feats^T @ dcls and dbias (num_classes) = sum_rows dcls: partials per 256-row tile (four 64-row groups in ascending row order, the groups
 * in ascending order), the tiles added in ascending order; these sums over all rows are kept in double (the products are exact there)
 * and rounded to fp32 once.  Each output optional (NULL).  C: a multiple of 64 up to 512;
 * 1 <= num_classes <= 16.  workspace: ptx_neck_head_bwd_workspace_bytes(n, C, num_classes) bytes (0: unsupported), for dweight / dbias. */
PTX_API size_t ptx_neck_head_bwd_workspace_bytes(int n, int C, int num_classes);
PTX_API int ptx_neck_head_bwd(const float *dcls, const float *feats, const float *weight, int n, int C, int num_classes, float *dfeats,
                      float *dweight, float *dbias, void *workspace, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ query selection behind the neck (ABI 13, by addition)
 * `pre_decoder` of the detector (detectors/sparse_featfusion_grounder_preshape.py:498-580): the neck's per-scene lists become the
 * transformer decoder's operands.  Assembled in Python (proxytransformation_amd/query_select.py), restated in numpy
 * (query_select_host.py).  fp32; no float atomics and fixed summation orders: two calls on the same inputs give the same bits;
 * everything on `stream`, no host wait; host checks (PTX_EINVAL with the numbers in the message) come before anything is enqueued.
 * rows: [host] B ints, the rows L_b of every scene, 0 <= L_b <= Lmax; B <= 64; C a multiple of 64 up to 512; 1 <= T <= 256;
 * masks are bytes of 0 / 1 (torch.bool).
 *
 * Pack: feats / xyz are [host] arrays of B device pointers, (L_b,C) and (L_b,3).  out_feats (B,Lmax,C) and out_coords (B,Lmax,3) get the
 * rows with zeros behind them, pad_mask (B,Lmax) = 1 on padding, text_attn (B,T) = !text_mask.  One launch. */
PTX_API int ptx_qs_pack(const float *const *feats, const float *const *xyz, const int32_t *rows, int B, int C, int Lmax,
                        const uint8_t *text_mask, int T, float *out_feats, float *out_coords, uint8_t *pad_mask, uint8_t *text_attn,
                        void *stream);
/* ContrastiveEmbed and its max over the tokens (grounding_head.py:62-99): score (B,Lmax), score[b,r] = max over the tokens t with
 * text_mask[b,t] of (feats[b,r] . text[b,t]) (/ sqrtf(C) when scaled) (+ bias[0] when bias is given); -inf for r >= rows[b] and for a
 * scene without a token; NaN where one of the unmasked products is NaN (torch.max's rule).  The product runs on the exact-fp32 matrix
 * instruction, 64 rows x 64 tokens per step; the (B,L,T) tensor is never materialised.  One launch. */
PTX_API int ptx_qs_score(const float *feats, const int32_t *rows, int B, int Lmax, int C, const float *text, const uint8_t *text_mask, int T,
                         int scaled, const float *bias, float *score, void *stream);
/* torch.topk(score, K, dim=1, sorted=True)[1] over the rows 0 .. rows[b] - 1 of every scene, 1 <= K <= 1024, K <= rows[b]: index (B,K)
 * int64 in descending order of ptx_neck_topk_prune's key (-0.0 = +0.0; a NaN orders by its bits), the lower row first among equal keys
 * (torch leaves ties unspecified).  inv (B,Lmax) int32, optional: the place q of a selected row, -1 elsewhere.  A radix select and a
 * sort of K (key, row) pairs in LDS, one work-group per scene.  One launch. */
PTX_API int ptx_qs_topk(const float *score, const int32_t *rows, int B, int Lmax, int K, int64_t *index, int32_t *inv, void *stream);
/* out (B K,Cout) = act(rows @ weight^T + bias) with weight (Cout,Cin) as nn.Linear holds it: row b K + q is x[b Lmax + index[b,q]] (x of
 * n_src rows; an index outside 0 .. Lmax - 1 reads zeros), or x[b K + q] when index is NULL.  relu: 0 / 1; the ReLU keeps a NaN.  Cin,
 * Cout: multiples of 64 up to 512.  The gather-GEMM of ptx_sparse_conv3d's transposed-weight form.  One launch. */
PTX_API int ptx_qs_linear(const float *x, int n_src, const int64_t *index, int B, int K, int Lmax, const float *weight, const float *bias,
                          int Cin, int Cout, int relu, float *out, void *stream);
/* The last Linear of the regression branch, weight (9,C) / bias (9), on h (B K,C) (NULL: on the gathered features), the baseline box
 * decode (grounding_head.py:293-297: center = p[0:3] + coords, size = max(expf(p[3:6]), 0.02) with a NaN kept, euler = p[6:9]) and the
 * gathers query (B,K,C) = feats[b, index], qcoords (B,K,3) = coords[b, index]; boxes (B,K,9).  One launch. */
PTX_API int ptx_qs_decode(const float *h, const float *weight, const float *bias, int C, const float *feats, const float *coords,
                          const int64_t *index, int B, int K, int Lmax, float *query, float *qcoords, float *boxes, void *stream);
/* The backward of pack + gather: out (sum of rows,C), scene b from row rows[0] + .. + rows[b-1]: out_b[r] = dfeats[b,r] (+ dquery[b,q]
 * where inv[b,r] = q >= 0: one fp32 add).  dfeats (B,Lmax,C) and dquery (B,K,C) are optional (NULL: zeros).  One launch. */
PTX_API int ptx_qs_bwd(const float *dfeats, const float *dquery, const int32_t *inv, const int32_t *rows, int B, int Lmax, int K, int C,
                       float *out, void *stream);

/* ------------------------------------------------------------------ the transformer decoder behind the query selection (ABI 13, by addition)
 * The eval forward of SparseFeatureFusionTransformerDecoder (models/layers/ground_transformer/decoder.py) and the per-layer text scores of
 * GroundingHead.forward, assembled in Python (proxytransformation_amd/decoder.py), restated in numpy (decoder_host.py).  fp32 on the
 * exact-fp32 matrix instruction; no float atomics and fixed summation orders: two calls on the same inputs give the same bits; everything
 * on `stream`, no host wait; host checks (PTX_EINVAL with the numbers in the message) come before anything is enqueued.  Masks are bytes
 * of 0 / 1 (torch.bool).
 *
 * PositionEmbeddingLearned in eval: out (n,C) = relu(x @ w1^T + b1) @ w2^T + b2 with x (n,cin), 1 <= cin <= 9, w1 (C,cin) / b1 (C) the
 * first Conv1d with the BatchNorm folded in by the caller, w2 (C,C) / b2 (C) the second; the ReLU keeps a NaN.  One launch. */
PTX_API int ptx_dec_posembed(const float *x, long n, int cin, const float *w1, const float *b1, const float *w2, const float *b2, int C,
                             float *out, void *stream);
/* out (n,Cout) = act((x + add) @ weight^T + bias) (+ residual) with weight (Cout,Cin) as nn.Linear holds it.  add (n,Cin), optional, is
 * added to x for the output columns below add_cols only (a multiple of 64): one launch gives [q|k|v] with the positions on q and k.
 * bias (Cout) and residual (n,Cout) are optional; relu: 0 / 1, applied before the residual, keeps a NaN.  Cin: a multiple of 64 up to
 * 2048; Cout: a multiple of 64 up to 4096.  One launch. */
PTX_API int ptx_dec_linear(const float *x, const float *add, int add_cols, long n, const float *weight, const float *bias, int Cin, int Cout,
                           int relu, const float *residual, float *out, void *stream);
/* Multi-head attention with a key padding mask: out (B,Kq,H hd) = softmax((q / sqrtf(hd)) k^T) v per head.  q (B,Kq,.) / k, v (B,L,.) may
 * be column ranges of wider rows: ldq / ldk / ldv are the row strides in floats (multiples of 4), scene b starts Kq ldq resp. L ldk / L ldv
 * floats behind scene b - 1, head h at column h hd.  mask (B,L), optional (NULL: none): 1 = ignore the key; a masked key and its value are never read (a NaN
 * under them leaves no trace), a query whose every key is masked gets zeros.  hd: 32 or 64; H hd <= 512; Kq <= 1024.  One launch: key
 * tiles of 64 in ascending order with a running maximum and sum. */
PTX_API int ptx_dec_attention(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B,
                              int Kq, int L, int H, int hd, float *out, void *stream);
/* out (n,C) = LayerNorm(x) with weight / bias (C): the row mean first, then the centred sum of squares.  weight2 / bias2 / out2, optional
 * (all or none): out2 = LayerNorm2(out).  C: a multiple of 64 up to 512.  One launch. */
PTX_API int ptx_dec_ln(const float *x, long n, int C, const float *weight, const float *bias, float eps, float *out, const float *weight2,
                       const float *bias2, float *out2, void *stream);
/* The last Linear of a regression branch, weight (9,C) / bias (9), on h (n,C) and ptx_qs_decode's baseline box decode against
 * coords (n,3): boxes (n,9).  One launch. */
PTX_API int ptx_dec_boxes(const float *h, const float *weight, const float *bias, int C, const float *coords, long n, float *boxes,
                          void *stream);
/* ContrastiveEmbed in full (grounding_head.py:62-99): out (NL,B,K,max_text_len), out[l,b,q,t] = hidden[l,b,q] . text[b,t] (/ sqrtf(C) when
 * scaled) (+ bias[0] when bias is given) for t < T with text_mask[b,t], -inf elsewhere.  One launch. */
PTX_API int ptx_dec_scores(const float *hidden, int NL, int B, int K, int C, const float *text, const uint8_t *text_mask, int T,
                           int max_text_len, int scaled, const float *bias, float *out, void *stream);

/* ------------------------------------------------------------------ the decoder's operators under autograd (ABI 13, by addition)
 * The backward of ptx_dec_attention and ptx_dec_ln (csrc/decoder_bwd.hip); the Linear's backward is ptx_op_gemm / ptx_op_colsum /
 * ptx_op_eltwise, assembled in Python (proxytransformation_amd/decoder.py), restated in numpy (decoder_grad_host.py).  The same rules:
 * fp32, no float atomics, fixed summation orders, everything on `stream`, no host wait, host checks before anything is enqueued.
 *
 * ptx_dec_attention with one more result: stats (B,H,Kq,2) = the final maximum and sum (m, l) of every (scene, head, query); l == 0 marks
 * a query without a key (m = -inf).  The same kernel and the same bits in `out` as ptx_dec_attention. */
PTX_API int ptx_dec_attention_stats(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B,
                                    int Kq, int L, int H, int hd, float *out, float *stats, void *stream);
/* The gradients of ptx_dec_attention: with P = expf((q / sqrtf(hd)) k^T - m) / l recomputed from stats, D = rowsum(dout * out),
 * dP = dout v^T, dS = P (dP - D): dv = P^T dout, dq = dS k / sqrtf(hd), dk = dS^T q / sqrtf(hd).  out, dout, dq (B,Kq,H hd) and dk, dv
 * (B,L,H hd) are dense; q, k, v and their strides as in the forward.  Every element of dq, dk, dv is written exactly once (no memset by
 * the caller): zeros for a masked key (never read, here either), for every key of a scene whose queries have no key and for the dq of a
 * query without a key.  rowdot: (B,H,Kq) floats of workspace (D).  Two launches: queries x key tiles ascending for dq, keys x query tiles
 * ascending for dk / dv. */
PTX_API int ptx_dec_attention_bwd(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B,
                                  int Kq, int L, int H, int hd, const float *out, const float *stats, const float *dout, float *dq,
                                  float *dk, float *dv, float *rowdot, void *stream);
/* The gradients of ptx_dec_ln at x (n,C): mean and rstd are recomputed as the forward computes them.  One norm (weight2 NULL): dy (n,C)
 * is the gradient of out; dx = LN^T(dy), xdy = xhat * dy; dweight = colsum(xdy), dbias = colsum(dy) (ptx_op_colsum).  Two norms
 * (weight2 given, with bias, g1 and xdy2): dy and dy2 are the gradients of out and out2, either may be NULL (zeros), not both;
 * g1 = dy + LN2^T(dy2), dx = LN^T(g1), xdy = xhat * g1, xdy2 = xhat2 * dy2; dweight = colsum(xdy), dbias = colsum(g1),
 * dweight2 = colsum(xdy2), dbias2 = colsum(dy2).  C: a multiple of 64 up to 512.  One launch. */
PTX_API int ptx_dec_ln_bwd(const float *x, long n, int C, const float *weight, const float *bias, float eps, const float *weight2,
                           const float *dy, const float *dy2, float *dx, float *xdy, float *g1, float *xdy2, void *stream);

/* ------------------------------------------------------------------ training through the whole decoder (ABI 13, by addition)
 * What ptx_dec_attention_bwd / ptx_dec_ln_bwd leave open (csrc/decoder_train.hip): PositionEmbeddingLearned with a training-mode
 * BatchNorm, the backward of ptx_dec_boxes and of ptx_dec_scores; restated in numpy by decoder_grad_host.py.  The same rules: fp32, no
 * float atomics, fixed summation orders, everything on `stream`, no host wait, host checks before anything is enqueued.  Sums over rows
 * run in double over slabs of rows that are added in ascending order; their workspace is
 * ptx_dec_train_workspace_bytes(n, C, nv) bytes (8-byte aligned) for nv values per channel: 0 where n (1 to 2^24), C (a multiple of 64
 * up to 512) or nv (1 to 10) is out of range. */
PTX_API size_t ptx_dec_train_workspace_bytes(long n, int C, int nv);
/* The batch statistics of z = x w1^T + b1 over the n >= 2 rows of x (n,cin), 1 <= cin <= 9, w1 (C,cin): mean and centred sum of squares
 * per channel (row slabs merged with Chan's formula in double), then, per channel in double and rounded once: rstd = 1 / sqrt(M2 / n +
 * eps), w1f = w1 gamma rstd, b1f = (b1 - mean) gamma rstd + beta -- the operands ptx_dec_posembed then takes -- and stats (2,C) =
 * (mean | rstd).  run_mean / run_var (both or neither): `repeat` sequential fp32 updates r = (1 - momentum) r + momentum v with the batch
 * mean and the unbiased variance M2 / (n - 1).  Workspace: nv = 2.  Two launches. */
PTX_API int ptx_dec_posembed_stats(const float *x, long n, int cin, const float *w1, const float *b1, const float *gamma, const float *beta,
                                   int C, double eps, float momentum, int repeat, float *run_mean, float *run_var, float *w1f, float *b1f,
                                   float *stats, void *workspace, size_t ws_bytes, void *stream);
/* h (n,C) = relu(x w1f^T + b1f): the hidden tensor of ptx_dec_posembed, its bits (the ReLU keeps a NaN).  One launch. */
PTX_API int ptx_dec_posembed_hidden(const float *x, long n, int cin, const float *w1f, const float *b1f, int C, float *h, void *stream);
/* The first layer's and the BatchNorm's gradients from dh (n,C), the gradient of the hidden tensor: dpre = dh where the recomputed hidden
 * value is > 0 (a NaN passes nothing), zhat = (z - mean) rstd; dgb (2,C) = (dbeta = sum dpre | dgamma = sum dpre zhat);
 * dz = gamma rstd (dpre - dbeta / n - zhat dgamma / n); dw1 (C,cin) = dz^T x, db1 (C) = sum dz.  Workspace: nv = max(cin + 1, 2).  Four
 * launches. */
PTX_API int ptx_dec_posembed_bwd(const float *x, long n, int cin, const float *w1, const float *b1, const float *gamma, const float *stats,
                                 const float *w1f, const float *b1f, const float *dh, int C, float *dgb, float *dw1, float *db1,
                                 void *workspace, size_t ws_bytes, void *stream);
/* The gradients of ptx_dec_boxes under dboxes (n,9): p = h weight^T + bias recomputed as the forward forms it; dp (n,9) = dboxes on the
 * centre and the angles, (expf(p) >= 0.02 ? dboxes : 0) * expf(p) on the sizes (torch's exp().clamp(min=0.02): NaN where p is NaN);
 * dh (n,C) = dp weight, dweight (9,C) = dp^T h.  dbias = the column sums of dp (ptx_op_colsum).  Workspace: nv = 9.  Three launches. */
PTX_API int ptx_dec_boxes_bwd(const float *h, const float *weight, const float *bias, int C, long n, const float *dboxes, float *dh, float *dp,
                              float *dweight, void *workspace, size_t ws_bytes, void *stream);
/* The gradients of ptx_dec_scores under dscores (NL,B,K,max_text_len), read only at the tokens t < T with text_mask[b,t] (a NaN elsewhere
 * leaves no trace): dhidden (NL,B,K,C) = dscores text (/ sqrtf(C) when scaled), dtext (B,T,C) = sum over (layer, query) ascending of
 * dscores^T hidden (/ sqrtf(C)), zeros on a masked token; dbias (1), optional = sum of dscores, per (layer, scene) in double and then
 * ascending, with NL B doubles of workspace.  Two launches, four with dbias. */
PTX_API int ptx_dec_scores_bwd(const float *dscores, const float *hidden, int NL, int B, int K, int C, const float *text,
                               const uint8_t *text_mask, int T, int max_text_len, int scaled, float *dhidden, float *dtext, float *dbias,
                               void *workspace, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ the grounding loss behind the decoder (ABI 13, by addition)
 * GroundingHead.loss as the shipped configuration runs it (dense_heads/grounding_head.py:606-824): the matching costs of
 * HungarianAssigner3D, the sigmoid focal loss over the unmasked text tokens and the decoupled corner (Chamfer) loss of the matched boxes,
 * forward and backward; assembled in Python (proxytransformation_amd/grounding_loss.py), restated in numpy (grounding_loss_host.py).
 * fp32; no float atomics and fixed summation orders: two calls on the same inputs give the same bits; everything on `stream`, no host
 * wait; host checks (PTX_EINVAL with the numbers in the message) come before anything is enqueued.  A box is (cx,cy,cz, sx,sy,sz,
 * a0,a1,a2) with R = Rz(a0) Rx(a1) Ry(a2) and the corners c + R (+-s/2).  Masks are bytes of 0 / 1 (torch.bool): 1 = a real token.
 *
 * out (N,M) = vol(A n B) / (vol A + vol B - vol(A n B)) of boxes1 (N,9) against boxes2 (M,9): the exact intersection volume of the two
 * hexahedra, coplanar faces decided once per pair of faces (grounding_loss_host.py states the rule); NaN for a box with a NaN, an inf or
 * a non-positive size.  One launch. */
PTX_API int ptx_gl_iou(const float *boxes1, int N, const float *boxes2, int M, float *out, void *stream);
/* cost (NL,K,SG): cost[l,q,g] = w_cls BinaryFocalLossCost(scores[l,b,q], positive_maps[g]) + w_l1 |boxes[l,b,q] - gt_boxes[g]|_1
 * - w_iou IoU(boxes[l,b,q], gt_boxes[g]) with b = gt_scene[g]: scores (NL,B,K,M), boxes (NL,B,K,9), text_mask (B,T), gt_boxes (SG,9),
 * positive_maps (SG,M), gt_scene (SG) on the device.  The focal cost runs over the tokens t < T with text_mask[b,t]; a masked token or a
 * column from T on is never read.  One launch. */
PTX_API int ptx_gl_cost(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T,
                        const float *gt_boxes, const float *positive_maps, const int32_t *gt_scene, int SG, float alpha, float gamma,
                        float w_cls, float w_l1, float w_iou, float *cost, void *stream);
/* losses (2,NL): losses[0][l] = cls_scale sum of the focal loss of layer l over its queries and unmasked tokens, with the target row
 * positive_maps[gt_offset[b] + assign[l,b,q]] or zeros where assign (NL,B,K) is -1; losses[1][l] = box_weight / (8 P_l) times the sum
 * over the P_l matched queries of the four Chamfer terms weighted by decouple_weights (4 floats on the host).  gt_offset (B+1) on the
 * device: scene b's boxes are the rows gt_offset[b] .. gt_offset[b+1] - 1.  rows: 2 NL B K floats of scratch; counts (NL): P_l.  Two
 * launches. */
PTX_API int ptx_gl_loss_fwd(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T,
                            const float *gt_boxes, const float *positive_maps, const int32_t *gt_offset, int SG, const int32_t *assign,
                            float alpha, float gamma, const float *decouple_weights, float cls_scale, float box_weight, float *rows,
                            float *losses, int32_t *counts, void *stream);
/* dscores (NL,B,K,M), dboxes (NL,B,K,9): the gradients of sum_l g_cls[l] losses[0][l] + g_box[l] losses[1][l] (g_cls, g_box (NL) on the
 * device, NULL: ones); counts as ptx_gl_loss_fwd left it.  Exactly 0 on a masked token, from column T on, and in the box of an unmatched
 * query.  One launch. */
PTX_API int ptx_gl_loss_bwd(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T,
                            const float *gt_boxes, const float *positive_maps, const int32_t *gt_offset, int SG, const int32_t *assign,
                            float alpha, float gamma, const float *decouple_weights, float cls_scale, float box_weight, const float *g_cls,
                            const float *g_box, const int32_t *counts, float *dscores, float *dboxes, void *stream);
/* out (n) = max_t sigmoid(scores[r,t]) over all M columns of scores (n,M): a -inf column gives 0, a NaN gives NaN.  One launch. */
PTX_API int ptx_gl_predict(const float *scores, long n, int M, float *out, void *stream);
/* assign (NL,B,K) int32 = the minimum-cost matching of every (layer, scene): the index of query k's box within its scene, -1 for an
 * unmatched query and for every query of a scene without a box.  cost (NL,K,SG) as ptx_gl_cost leaves it (a NaN or +inf entry counts as
 * 100, -inf as -100); scene b's K x G_b matrix is the columns gt_offset[b] .. gt_offset[b+1] - 1 (gt_offset (B+1) on the device); max_g
 * = the host's max_b G_b.  The rectangular shortest-augmenting-path method in double, one wave per problem; min(K, G_b) pairs; among
 * columns of equal smallest path cost the lowest index is taken (grounding_loss_host.sap_assign_host is the specification, bit for bit).
 * Limits: min(K, max_g) <= 256, max(K, max_g) <= 1024.  A scene whose offsets are not 0 <= lo <= hi <= SG with hi - lo <= max_g reads
 * nothing and gets -1.  assign is written entirely (no memset needed).  One launch; added without a change of the ABI version. */
PTX_API int ptx_gl_assign(const float *cost, int NL, int B, int K, const int32_t *gt_offset, int SG, int max_g, int32_t *assign,
                          void *stream);

/* ------------------------------------------------------------------ image feature -> point sampling
 * batch_point_sample (models/layers/fusion_layers/point_fusion.py:208-313) as called at detectors/
 * sparse_featfusion_grounder_preshape.py:428-444 (nearest, zeros padding, align_corners=True, valid_flag=True; bilinear != 0:
 * the function's own default aligned=True, F.grid_sample(mode='bilinear'), neighbours outside the map count as 0):
 * out (N,C) = sum over ALL V views of the sampled feature pixel / max(#views in which the point is inside the padded
 * image with depth > 0, 1), zero rows where that count is 0.  feats (V,C,H,W) fp32 / bf16 / fp16 (feat_dtype 0/1/2);
 * proj (V,4,4) row-major = intrinsic @ extrinsic; pre: optional (3,4) affine applied to the points first (the reverse
 * 3D augmentation of apply_3d_transformation, composed by the host) or NULL; image transform scale -> crop -> flip
 * (flip: x = ori_w - x); pad_h / pad_w: padded image size.  workspace: ptx_point_sample_workspace_bytes() bytes (one
 * channels-last copy of the feature maps).  valid_num (N) int32 optional. */
PTX_API size_t ptx_point_sample_workspace_bytes(int V, int C, int H, int W);
/* ABI 12: the channels-last copy of the feature maps alone (what ptx_point_sample does first), e.g. on another stream while the
 * points are still being produced; ptx_point_sample(feats = NULL, ...) then samples from the prepared workspace. */
PTX_API int ptx_point_sample_prepare(const void *feats, int feat_dtype, int V, int C, int H, int W, void *workspace, size_t ws_bytes,
                             void *stream);
PTX_API int ptx_point_sample(const float *points, int N, const void *feats, int feat_dtype, int V, int C, int H, int W,
                     const float *proj, const float *pre, float scale_w, float scale_h, float crop_w, float crop_h, int flip,
                     float ori_w, float pad_h, float pad_w, int bilinear, float *out, int32_t *valid_num, void *workspace,
                     size_t ws_bytes, void *stream);
/* The backward of ptx_point_sample with respect to the feature maps (ABI 13, by addition).  The forward is linear in them, so
 *   dfeats[v, c, y, x] = sum over the (point n, view v) pairs whose sample touches that pixel of  w * (dout[n, c] / valid_num[n]),
 * w = 1 (nearest) or the neighbour's bilinear weight as the forward forms it; only points with valid_num[n] > 0 contribute, through
 * every view whose sample is inside the map (valid or not, like the forward).  dout (N,C) fp32; valid_num (N): what the forward
 * wrote; dfeats (V,C,H,W) in storage type feat_dtype: EVERY element is written exactly once (zeros where nothing lands; no
 * memset by the caller), the sum is kept in fp32 in ascending point order and rounded once on the store -- no float atomics,
 * bitwise reproducible.  The index is rebuilt from points / proj / pre / the image transform (the arguments of the forward);
 * nothing of the forward needs saving but valid_num.  The points get no gradient.  workspace: ptx_point_sample_bwd_workspace_bytes()
 * bytes, sized for the worst case N * V (* 4 neighbours) list entries; 0 when a size is outside the supported range.  All checks
 * are on the host, before anything is enqueued: PTX_EINVAL / PTX_ENOSPACE with a message. */
PTX_API size_t ptx_point_sample_bwd_workspace_bytes(int N, int V, int H, int W, int bilinear);
PTX_API int ptx_point_sample_bwd(const float *points, int N, const float *dout, const int32_t *valid_num, int V, int C, int H, int W,
                         const float *proj, const float *pre, float scale_w, float scale_h, float crop_w, float crop_h, int flip,
                         float ori_w, float pad_h, float pad_w, int bilinear, void *dfeats, int feat_dtype, void *workspace,
                         size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ level join (ABI 13, by addition)
 * detectors/sparse_featfusion_grounder_preshape.py:428-479 for ONE backbone level and every scene at once: each row of a sparse
 * level gets the image features sampled at its position appended,
 *   out[r] = [ level_feats[r] (Cb) | ptx_point_sample of scene coords[r,0] at (float)coords[r,1:4] * voxel_size (Ci) ],
 * in one launch.  coords (n,4) int32 rows (scene, x, y, z), the rows of a scene contiguous and the scenes ascending; the point is one
 * rounded multiply, the bits ptx_voxel_coarsen emits; the sampling is the arithmetic of ptx_point_sample itself (shared device
 * functions), so out[:, Cb:] equals the per-scene calls bit for bit, nearest (bilinear = 0) and bilinear.  featT: a HOST array of B
 * device pointers, scene b's channels-last maps as ptx_point_sample_prepare wrote them ((V, H*W, Ci) fp32), read in place.
 * tables: ptx_level_join_table_floats(B, V) floats, the same content on the host (tables_host: read by the checks) and on the
 * device (tables_dev: read by the kernels; the caller uploads it, e.g. one pinned staging copy for all levels):
 *   scene b at tables + 32 b:  [0:12] the (3,4) pre-transform, [12] != 0: apply it, [13] scale_w, [14] scale_h, [15] crop_w,
 *                              [16] crop_h, [17] != 0: flip, [18] ori_w, [19] pad_h, [20] pad_w, [21:32] unused
 *   then proj (B, V, 4, 4) row-major at tables + 32 B.
 * V is the same for every scene.  Cb, Ci: multiples of 64 up to 512; 1 <= B <= 64; n >= 0 (n == 0 launches nothing); a scene
 * without rows is fine; a row whose scene index is outside [0, B) gets zeros.  level_feats and out: 16-byte aligned.  valid_num (n) int32
 * or NULL.  All checks are on the
 * host, before anything is enqueued. */
PTX_API size_t ptx_level_join_table_floats(int B, int V);
PTX_API int ptx_level_join(const int32_t *coords, int n, const float *level_feats, int Cb, const float *const *featT,
                   const float *tables_host, const float *tables_dev, int B, int V, int Ci, int H, int W, float voxel_size,
                   int bilinear, float *out, int32_t *valid_num, void *stream);
/* The backward of ptx_level_join in one call.  g (n, Cb + Ci) fp32 contiguous, 16-byte aligned: dlevel_feats (n, Cb) = g[:, :Cb]
 * (NULL: not wanted); dimg (B, V, Ci, H, W) in storage type feat_dtype (NULL: not wanted) = ptx_point_sample_bwd of every scene on
 * g[rows of the scene, Cb:], read in place by leading dimension and column offset: the same inverted index, scene by scene on the
 * one workspace, every element written once (a scene without rows: zeros), no float atomics, bitwise reproducible.  scene_end: a
 * HOST array, scene b's rows are [scene_end[b-1], scene_end[b]), scene_end[B-1] = n.  valid_num: what the forward wrote.
 * workspace: ptx_level_join_bwd_workspace_bytes(the largest scene's rows, ...) bytes (0: outside the 32-bit index range; not
 * needed when dimg is NULL or n == 0). */
PTX_API size_t ptx_level_join_bwd_workspace_bytes(int max_rows, int V, int H, int W, int bilinear);
PTX_API int ptx_level_join_bwd(const int32_t *coords, int n, const int32_t *scene_end, const float *g, int Cb, const int32_t *valid_num,
                       const float *tables_host, const float *tables_dev, int B, int V, int Ci, int H, int W, float voxel_size,
                       int bilinear, float *dlevel_feats, void *dimg, int feat_dtype, void *workspace, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ train-mode operators
 * The differentiable half of the path in train mode -- batch-statistics BatchNorm2d / BatchNorm1d (PRE:74, 114,
 * 329-330), Dropout (PRE:189-191, timm Mlp), DropPath (PRE:268) and the gradients of everything between the ball
 * queries and the scatter -- as forward / backward kernel pairs.  The index half (ball query, FPS, selection, tags:
 * ptx_grid_centers, ptx_ball_query, ptx_select_clusters, ptx_affine_compact above) is shared with eval mode and is not
 * differentiable, as in the reference.  proxytransformation_amd/train.py chains these with torch.autograd.Function
 * nodes (torch keeps the graph and the buffers; every arithmetic step is one of these kernels).  All tensors dense
 * row-major fp32 unless noted; nothing synchronises the host. */

/* C[z][m][n] (+)= alpha * sum_k A[z][m][k] B[z][k][n] with arbitrary element strides (NN / NT / TN, head-split views,
 * channels-first image features: a_dtype / b_dtype 0 fp32, 1 bf16, 2 fp16); z = z1 * inner + z2, one stride per batch
 * digit.  ksplit > 1: K is cut into slices whose partial products land c_sk elements apart (summed by the caller with
 * ptx_op_colsum) -- weight gradients contract over every slot / token of the batch with a tiny M x N. */
PTX_API int ptx_op_gemm(const void *A, const void *B, float *C, int M, int N, int K, long a_rs, long a_cs, long b_rs, long b_cs,
                long c_rs, long c_cs, int batch, int inner, long a_s1, long a_s2, long b_s1, long b_s2, long c_s1, long c_s2,
                int a_dtype, int b_dtype, float alpha, int accumulate, int ksplit, long c_sk, void *stream);
/* The kernel the same ptx_op_gemm call would take, decided on the host (launches nothing, touches no device): 0 = k_bgemm (64 x 64
 * MFMA tiles), 1 = k_bthin_out, scalar requests, 2 = k_bthin_out, four k per request, 3 = k_bthin_row; PTX_EINVAL where ptx_op_gemm
 * refuses the arguments.  ptx_op_gemm dispatches on this very function.  (ABI 13, by addition.) */
PTX_API int ptx_op_gemm_route(const void *A, const void *B, const float *C, int M, int N, int K, long a_rs, long a_cs, long b_rs,
                long b_cs, long c_rs, long c_cs, int batch, int inner, long a_s1, long a_s2, long b_s1, long b_s2, long c_s1, long c_s2,
                int a_dtype, int b_dtype, float alpha, int accumulate, int ksplit, long c_sk);
/* out (cols,rows) = in (rows,cols)^T */
PTX_API int ptx_op_transpose(const float *in, int rows, int cols, float *out, void *stream);
/* out[n] (+)= scale * sum_r f(x[r][n]), accumulated in double; mode 0: x, 1: x*y, 2: x*x, 3: (x - y[n])^2 with y a
 * per-column vector (bias / LayerNorm / BatchNorm parameter gradients, batch statistics) */
PTX_API int ptx_op_colsum(const float *x, const float *y, int R, int N, int mode, float scale, int accumulate, float *out,
                  double *scratch /* nsplit * N doubles */, int nsplit, void *stream);
/* op 0: a+b  1: a*s  2: gelu(a)  3: b*gelu'(a)  4: relu(a)  5: b*(a>0)  6: a+bias[col]  7: a+s*b  8: a*b */
PTX_API int ptx_op_eltwise(int op, const float *a, const float *b, float s, long n, int ncol, float *y, void *stream);
/* y = x * keep / (1-p), keep = hash(seed, i / group) >= p: Dropout (group 1) / DropPath (group = elements per sample);
 * the backward pass is the same call on dy */
PTX_API int ptx_op_dropout(const float *x, long n, long group, float p, uint64_t seed, float *y, void *stream);
/* LayerNorm over C (+ optional per-slot bias table add[(row % add_rows)], PRE:215-217); stats (R,2) = mean, rstd */
PTX_API int ptx_op_layernorm_fwd(const float *x, const float *w, const float *b, const float *add, int add_rows, int R, int C,
                         float eps, float *y, float *stats, void *stream);
PTX_API int ptx_op_layernorm_bwd(const float *x, const float *w, const float *dy, const float *stats, int R, int C, float *dx,
                         float *xhat, void *stream);
/* BatchNorm over the rows of (R,C) with batch statistics: mean = colsum / R, centred sum of squares (colsum mode 3) ->
 * mean / rstd (+ running-stat update with momentum, unbiased variance) -> apply (optionally fused ReLU); backward in
 * three steps (see train_ops.hip) */
PTX_API int ptx_op_bn_stats(const float *mean, const float *sumsq_centred, int C, long R, float eps, float momentum, float *mean_rstd,
                    float *run_mean, float *run_var, void *stream);
PTX_API int ptx_op_bn_apply(const float *x, const float *mean_rstd, const float *w, const float *b, long R, int C, int relu, float *y,
                    void *stream);
PTX_API int ptx_op_bn_bwd_prep(const float *x, const float *y, const float *dy, const float *mean_rstd, long R, int C, int relu,
                       float *g, float *gx, void *stream);
PTX_API int ptx_op_bn_bwd_dx(const float *x, const float *g, const float *mean_rstd, const float *w, const float *dbeta,
                     const float *dgamma, long R, int C, float *dx, void *stream);
/* softmax over the last dim of (rows, L); mask (B,L) uint8 (1 = valid) fills -1e9 (PRE:247), row r -> scene r / rows_per_scene */
PTX_API int ptx_op_softmax_fwd(const float *s, const uint8_t *mask, long rows, int L, long rows_per_scene, float *p, void *stream);
PTX_API int ptx_op_softmax_bwd(const float *p, const float *dp, const uint8_t *mask, long rows, int L, long rows_per_scene, float *ds,
                       void *stream);
/* OffsetNetwork / SimplifiedPointNet pieces (PRE:87-107, 126-142): slot inputs [rel | p] with padded slots zeroed,
 * pooling over the K slots (mode 0 mean, 1 max), tanh * margin + add + clamp (dcoef = d centre / d raw) */
PTX_API int ptx_op_slot_inputs(const float *center, const float *cluster, const int32_t *src, long nclus, int K, float *x6,
                       uint8_t *padmask, void *stream);
PTX_API int ptx_op_slot_inputs_bwd(const float *dx6, const uint8_t *padmask, long nclus, int K, float *dcenter, void *stream);
PTX_API int ptx_op_slot_pool(const float *h, long nclus, int K, int C, int mode, float *out, int32_t *arg, void *stream);
PTX_API int ptx_op_slot_pool_bwd(const float *dout, const int32_t *arg, long nclus, int K, int C, int mode, float *dh, void *stream);
PTX_API int ptx_op_offset_apply(const float *c0, const float *raw, const float *minmax, long nclus, int M, float margin, float *cout,
                        float *dcoef, void *stream);
/* The same networks fused (csrc/slotnet_train.hip): slot inputs -> Conv2d(6,C,1) -> BatchNorm2d (batch statistics over all
 * nclus*K slots, running statistics updated) -> ReLU -> mean (maxpool 0) / max (1, first arg-max in arg) over the K slots,
 * recomputing the C channels of a slot from its six inputs in every pass instead of storing (nclus*K, C) activations.
 * center (nclus,3), cluster (nclus,K,3); out (nclus,C); mean_rstd (2,C) is saved for the backward; stat_tmp (2,C) scratch;
 * scratch: ptx_op_slotnet_scratch_bytes(C).  Backward: dout (nclus,C) -> dconv_w (C,6), dconv_b (C), dbeta_dgamma (2,C),
 * dcenter (nclus,3) or NULL. */
PTX_API size_t ptx_op_slotnet_scratch_bytes(int C);
PTX_API int ptx_op_slotnet_fwd(const float *center, const float *cluster, long nclus, int K, int C, const float *conv_w,
                       const float *conv_b, const float *bn_w, const float *bn_b, float eps, float momentum, float *run_mean,
                       float *run_var, int maxpool, float *out, int32_t *arg, float *mean_rstd, float *stat_tmp, void *scratch,
                       size_t scratch_bytes, void *stream);
PTX_API int ptx_op_slotnet_bwd(const float *center, const float *cluster, long nclus, int K, int C, const float *conv_w,
                       const float *conv_b, const float *bn_w, const float *bn_b, const float *mean_rstd, int maxpool,
                       const int32_t *arg, const float *dout, float *dconv_w, float *dconv_b, float *dbeta_dgamma,
                       float *dcenter, void *scratch, size_t scratch_bytes, void *stream);
/* per-slot bias table of ProxyAttention (PRE:212-215) and its parameter gradients */
PTX_API int ptx_op_slotbias_fwd(const float *pb, const float *pc, const float *pr, int Mk, int s, int C, float *table, void *stream);
PTX_API int ptx_op_slotbias_bwd(const float *dtable, int Mk, int s, int C, float *dpb, float *dpc, float *dpr, void *stream);
/* rows of the kept clusters: src[b*Mk+j] = b*M + order[b][keep[b][j]]; gather / scatter of (rows,C) by src */
PTX_API int ptx_op_keep_rows(const int32_t *order, const int32_t *keep, int B, int M, int Mt, int Mk, int32_t *src, void *stream);
PTX_API int ptx_op_rows_gather(const float *x, const int32_t *src, long rows, int C, float *y, void *stream);
PTX_API int ptx_op_rows_scatter(const float *dy, const int32_t *src, long rows, int C, float *dx, void *stream);
/* output position of every input point after remove_points_by_index (PRE:516-523), -1 = dropped, + survivor counts */
PTX_API int ptx_op_out_positions(const uint32_t *tag, int B, int N, int32_t *tile_counts, int32_t *opos, int32_t *counts, void *stream);
/* gradients of the per-cluster affine + pt_replace (PRE:459-465): every valid slot whose target point survives receives
 * that point's output gradient (index_put_ backward gathers; duplicates included) */
PTX_API int ptx_op_affine_bwd(const float *dout, const int32_t *opos, const int32_t *kidx, const float *kcluster,
                      const float *kcenter, const float *transform, int B, int N, int Mk, int K, float *dtranslate,
                      float *dtransform, float *dkcenter, void *stream);
/* the same with one gradient per scene (the module returns a LIST of (n_b,3) tensors, PRE:467): douts [host] = B <= 32 device
 * pointers, NULL where a scene's output received no gradient */
PTX_API int ptx_op_affine_bwd_list(const float *const *douts, const int32_t *opos, const int32_t *kidx, const float *kcluster,
                           const float *kcenter, const float *transform, int B, int N, int Mk, int K, float *dtranslate,
                           float *dtransform, float *dkcenter, void *stream);
/* AttentionPool2d tokens (PRE:155-157): token 0 = mean of the pixel tokens, then + positional embedding; backward of the mean */
PTX_API int ptx_op_tokens_finish(float *tok, const float *pos, int nimg, int hw, int C, void *stream);
PTX_API int ptx_op_tokens_finish_bwd(float *dtok, int nimg, int hw, int C, void *stream);

/* ---- one ProxyBlock of the training step as two calls (csrc/train_fused.hip)
 * ProxyBlock in train mode (PRE:273-276: x + DropPath(attn(norm1(x) [+ slot bias], proxy)), x + DropPath(mlp(norm2(x))))
 * followed by the trailing LayerNorm, the Linear head and its BatchNorm1d with batch statistics (PRE:441-446, 450-455):
 * the forward and the whole backward of that chain, each enqueued by ONE call (the step was host-bound at ~400 launches
 * issued one ctypes call at a time: r04, 4.9 ms of enqueue for 3.7 ms of kernels).  Inside: the tuned NT GEMMs of the
 * eval path, proxy attention forward / backward as five kernels (both soft-maxes, both dropouts and all eight
 * contractions), residual + Dropout + DropPath + LayerNorm in one pass, every bias / LayerNorm gradient as partial
 * column sums emitted by the kernel that produces the rows and summed in one fixed-order pass at the end.
 * rows R = B * n tokens (scene-major), proxies B * L; param[] / grad[] in the order of PTX_TB_*; a NULL qkv bias is
 * allowed (qkv_bias = False).  save: activations the backward needs; tmp: scratch (sizes from ptx_train_block_sizes;
 * the backward's tmp need not be the forward's).  seed[0..5]: the six dropout sites of train.site_seeds (the
 * attention maps use seed[0] and seed[0] + 1).  Proxy attention is fused for L * head_dim <= 4096. */
enum { PTX_TB_LN1_W = 0, PTX_TB_LN1_B, PTX_TB_PB, PTX_TB_PC, PTX_TB_PR, PTX_TB_QKV_W, PTX_TB_QKV_B, PTX_TB_PP_W,
       PTX_TB_PP_B, PTX_TB_PROJ_W, PTX_TB_PROJ_B, PTX_TB_LN2_W, PTX_TB_LN2_B, PTX_TB_FC1_W, PTX_TB_FC1_B, PTX_TB_FC2_W,
       PTX_TB_FC2_B, PTX_TB_LN3_W, PTX_TB_LN3_B, PTX_TB_HEAD_W, PTX_TB_HEAD_B, PTX_TB_BN_W, PTX_TB_BN_B, PTX_TB_NPARAM };
typedef struct {
    int32_t B, n, L, C, H, heads, s, nout;     /* s: bias grid side (pc / pr), nout: head width (3 / 9) */
    int32_t compute_dtype;                     /* 0: fp32-equivalent products (three-way bf16 split); 1: plain bf16 operands, fp32 accumulation, for the
                                                  five Linear layers of the block and their gradients (what autocast gives them under --amp) */
    float eps1, eps2, eps3, bn_eps, bn_momentum;
    float p_attn, p_drop, p_path;
    uint64_t seed[6];
    const float *x;                            /* (R, C) point proxies */
    const float *proxy;                        /* (B*L, C) */
    const uint8_t *mask;                       /* (B, L), 1 = valid, or NULL */
    const float *param[PTX_TB_NPARAM];
    float *bn_run_mean, *bn_run_var;           /* updated by the forward (momentum, unbiased variance) */
    float *out;                                /* forward: (R, nout) */
    float *save; size_t save_floats;
    float *tmp; size_t tmp_floats;
    /* backward only */
    const float *dout;                         /* (R, nout) */
    float *dx;                                 /* (R, C) */
    float *dproxy;                             /* (B*L, C) */
    float *grad[PTX_TB_NPARAM];                /* shaped like param[] */
    const float *dx_add;                       /* optional (R, C): added into dx (the other block's gradient of the same point proxies) */
} PtxTrainBlock;
PTX_API int ptx_train_block_sizes(const PtxTrainBlock *a, size_t *save_floats, size_t *tmp_fwd_floats, size_t *tmp_bwd_floats);
PTX_API int ptx_train_block_fwd(const PtxTrainBlock *a, void *stream);
PTX_API int ptx_train_block_bwd(const PtxTrainBlock *a, void *stream);
/* the attention core alone (train._ProxyAttnCore): qkv (B*n,3C), pt (B*L,C) -> o (B*n,C), saving P1 (B,heads,L,n),
 * PV (B,heads,L,hd), P2 (B,heads,n,L); backward -> dqkv, dpt; tmp: ptx_train_attn_tmp_floats() floats.  Returns
 * PTX_EINVAL when the shape is outside the fused range (the caller falls back to the generic products). */
PTX_API size_t ptx_train_attn_tmp_floats(int B, int n, int L, int heads, int C);
PTX_API int ptx_train_attn_fwd(const float *qkv, const float *pt, const uint8_t *mask, int B, int n, int L, int heads, int C,
                       float p_drop, uint64_t seed, float *P1, float *PV, float *P2, float *o, void *stream);
PTX_API int ptx_train_attn_bwd(const float *qkv, const float *pt, const uint8_t *mask, int B, int n, int L, int heads, int C,
                       float p_drop, uint64_t seed, const float *P1, const float *PV, const float *P2, const float *dO,
                       float *dqkv, float *dpt, float *tmp, size_t tmp_floats, void *stream);

/* backward of a narrow Linear without bias, y (R, nout <= 9) = x (R, C) w^T (the offset network's channel_mapper, PRE:75; the
 * blocks' heads use the same kernel inside ptx_train_block_bwd): dx = (dt * coef) w, dw = (dt * coef)^T x; coef (R, nout) or NULL;
 * tmp: ptx_op_head_bwd_tmp_floats() floats (per-chunk partials of dw, summed in chunk order) */
PTX_API size_t ptx_op_head_bwd_tmp_floats(int R, int C, int nout);
PTX_API int ptx_op_head_bwd(const float *dt, const float *coef, const float *x, const float *w, int R, int C, int nout, float *dx, float *dw,
                    float *tmp, size_t tmp_floats, void *stream);

/* ---- AttentionPool2d in train mode without materialised pixel tokens (csrc/train_img.hip; PRE:144-177, 338)
 * img (nimg, Cin, hw) in its storage type (img_dtype 0 fp32 / 1 bf16 / 2 fp16) -> o (nimg, C), the attention output of the
 * one query that is returned (token 0), BEFORE c_proj; wc / bc: channel_mapper (C, Cin), (C); pos: positional_embedding
 * (hw + 1, C); wq .. bv: q_proj / k_proj / v_proj.  Because only token 0 queries, keys, values and every gradient collapse
 * onto `heads` vectors per image: two streaming passes over img forward, two backward (+ one write of dimg), all other
 * products a few hundred rows.  heads must be 8, hw <= 256, Cin % 8 == 0, Cin <= 2048, C <= 512.  The backward needs the
 * forward's `save`; dimg may be NULL (features without gradient).  dbk is the rounding-level zero the reference produces
 * too (the soft-max gradient sums to zero). */
typedef struct {
    int32_t nimg, Cin, hw, C, heads, img_dtype;
    const void *img;
    const float *wc, *bc, *pos, *wq, *bq, *wk, *bk, *wv, *bv;
    float *o;
    float *save; size_t save_floats;
    float *tmp; size_t tmp_floats;
    const float *dout;                         /* backward: (nimg, C) */
    void *dimg;                                /* (nimg, Cin, hw) in img's storage type, or NULL */
    float *dwc, *dbc, *dpos, *dwq, *dbq, *dwk, *dbk, *dwv, *dbv;
    /* optional tail (cw != NULL): proxy = LayerNorm(o cw^T + cb) -- c_proj and norm_img (PRE:177, 450) in the same two calls; the
     * forward then writes `proxy` (nimg, C) (o may be NULL: it lives in `save`), the backward takes `dproxy` instead of dout */
    const float *cw, *cb, *lnw, *lnb; float ln_eps;
    float *proxy;
    const float *dproxy;
    float *dcw, *dcb, *dlnw, *dlnb;
} PtxTrainImgPool;
PTX_API int ptx_train_imgpool_sizes(const PtxTrainImgPool *a, size_t *save_floats, size_t *tmp_fwd_floats, size_t *tmp_bwd_floats);
PTX_API int ptx_train_imgpool_fwd(const PtxTrainImgPool *a, void *stream);
PTX_API int ptx_train_imgpool_bwd(const PtxTrainImgPool *a, void *stream);

/* ---- the whole training step as ONE call per direction (ABI 12, csrc/train_step.hip; VERDICT r05 "next" #4)
 * Train-mode forward of the module (PRE:424-469 with batch-statistics BatchNorm, Dropout / DropPath) and its whole backward, each
 * enqueued by one call: the index half (grid centres, both ball queries, selection, tags, output positions), the two slot networks,
 * the folded attention pool with c_proj + norm_img, the two ProxyBlocks with their heads, and the affine apply with compaction --
 * what proxytransformation_amd/train.py's one-node step used to chain from Python with ~35 library calls and ~60 allocations.
 * The host side keeps the autograd node and the ALLOCATIONS: the library carves every intermediate out of caller-owned arenas
 * whose sizes and named offsets ptx_train_step_layout() reports (a pure function of the shape fields).
 *
 * caller fills: shape; points (B,N,3) stacked; lin; text_feats / text_mask; off / enc / map_w; ip (sizes, img, parameters, tail
 * parameters); tb / ib (sizes, scalars, seeds, mask, parameters, running statistics -- x / proxy / out / save / tmp are set by the
 * library); ws (the lane workspace: ptx_workspace_bytes / _init, for the compaction); out (B,N,3); counts_host (B int32, pinned);
 * arena_fwd; the optional side stream with four events (fork / join / pp / counts; any hipEvent_t, used in that role only inside
 * the two calls).  The forward copies the per-scene survivor counts to counts_host and records ev_counts behind the copy: wait for
 * that event, then out[b, :counts[b]] are scene b's rows (PRE:467).  ptx_train_step_bwd additionally takes douts (a [host] array of
 * B device pointers to the gradients of those rows), optional gradients of kcenter / translate / transform (return_transforms),
 * arena_bwd, grads (layout.grads_floats floats: every parameter gradient at layout.grad_off[...], shaped like the parameter) and
 * dtext (B*L,C) / dimg (in img's storage type) or NULL.  Gradient slots of the offset network's BatchNorm are [bias | weight]. */
typedef struct PtxTrainSlotNet {               /* Conv2d(6,W,1) + BatchNorm2d(W) of OffsetNetwork / SimplifiedPointNet (PRE:72-76, 112-116) */
    const float *conv_w, *conv_b, *bn_w, *bn_b;
    float *run_mean, *run_var;
    float eps, momentum;
    int32_t W;
} PtxTrainSlotNet;
enum { PTX_TS_OFF_CONV_W = 0, PTX_TS_OFF_CONV_B, PTX_TS_OFF_BN_W, PTX_TS_OFF_BN_B, PTX_TS_MAP_W,
       PTX_TS_ENC_CONV_W, PTX_TS_ENC_CONV_B, PTX_TS_ENC_BN_W, PTX_TS_ENC_BN_B,
       PTX_TS_IP0,                              /* wc bc pos wq bq wk bk wv bv cw cb lnw lnb */
       PTX_TS_TB0 = PTX_TS_IP0 + 13,            /* PTX_TB_* order */
       PTX_TS_IB0 = PTX_TS_TB0 + PTX_TB_NPARAM,
       PTX_TS_NGRAD = PTX_TS_IB0 + PTX_TB_NPARAM };
typedef struct PtxTrainStepLayout {
    size_t arena_fwd_bytes, arena_bwd_bytes, grads_floats;
    /* byte offsets of named regions of the forward arena (tests / return_transforms read them) */
    size_t idx2, order, picks, keep, kidx, drop_idx, centers, translate, transform, point_proxy, img_proxy, kcenter, opos;
    int64_t grad_off[PTX_TS_NGRAD];             /* float offsets into `grads`; -1: parameter absent (qkv bias) */
} PtxTrainStepLayout;
typedef struct PtxTrainStep {
    PtxShape shape;
    const float *points, *lin, *centers_override;
    const int32_t *order_override;
    const float *text_feats; const uint8_t *text_mask;
    PtxTrainSlotNet off, enc;
    const float *map_w;                         /* Conv1d(256,3,1,bias=False) weight (3,256) */
    PtxTrainImgPool ip;
    PtxTrainBlock tb, ib;
    void *ws; size_t ws_bytes;
    float *out; int32_t *counts_host;
    void *arena_fwd; size_t arena_fwd_bytes;
    void *side_stream; void *ev_fork, *ev_join, *ev_pp, *ev_counts;
    int32_t blocks_apart;                       /* the image block beside the text block on the side stream (forward and backward) */
    /* backward */
    const float *const *douts;
    const float *g_kcenter, *g_translate, *g_transform;
    void *arena_bwd; size_t arena_bwd_bytes;
    float *grads; size_t grads_floats;
    float *dtext; void *dimg;
} PtxTrainStep;
PTX_API int ptx_train_step_layout(const PtxTrainStep *a, PtxTrainStepLayout *out);
PTX_API int ptx_train_step_fwd(const PtxTrainStep *a, void *stream);
PTX_API int ptx_train_step_bwd(const PtxTrainStep *a, void *stream);

/* ------------------------------------------------------------------ the CLIP text encoder (ABI 13, by addition)
 * The eval forward of CLIPTextModel up to last_hidden_state (csrc/text_encoder.hip), restated in numpy by text_encoder_host.py: pre-norm
 * layers of width C = 64 H (up to 1280; head dimension 64 only), MLP width I (a multiple of 64 up to 5120) with quick-GELU, 1 <= T <= 256
 * tokens and no more than the position table holds, 1 <= B <= 64 texts; n = B T rows.  The same rules: fp32, no float atomics, fixed
 * summation orders (two calls give the same bits, and a row's bits do not depend on the other rows), everything on `stream`, no host
 * wait, host checks before anything is enqueued.
 *
 * out (B,T,C): out[b,t] = token_embedding[ids[b,t]] + position_embedding[t], ids (B,T) int64 on the device.  An id outside [0, vocab)
 * reads nothing and fills its row with NaN.  One launch. */
PTX_API int ptx_txt_embed(const long long *ids, int B, int T, const float *token_embedding, const float *position_embedding, int vocab,
                          int positions, int C, float *out, void *stream);
/* out (n,Cout) = act(LayerNorm(x) @ weight^T + bias) on x (n,Cin): per row the mean, then the centred variance, rstd = 1 / sqrtf(var + eps),
 * written once to stats (n,2) = (mean, rstd), workspace; (x - mean) rstd ln_weight + ln_bias applied in the operand load; act: 0 none,
 * 1 quick-GELU v / (1 + expf(-1.702 v)).  bias optional.  Cin: a multiple of 64 up to 1280; Cout: a multiple of 64 up to 5120.  Two
 * launches. */
PTX_API int ptx_txt_ln_linear(const float *x, long n, const float *ln_weight, const float *ln_bias, float eps, const float *weight,
                              const float *bias, int Cin, int Cout, int act, float *out, float *stats, void *stream);
/* Causal self attention of H heads of 64 on qkv (B,T,3 C) = [q|k|v]: out (B,T,C), heads merged.  q is scaled by 1/8; key j is admitted for
 * query t iff j <= t and mask[b,j] (mask (B,T), 1 = a token; NULL: every key is one).  A masked key is never read, a key tile without an
 * admitted key is skipped, a query without an admitted key gets zeros; every one of the T query rows is computed.  One launch. */
PTX_API int ptx_txt_attention(const float *qkv, const uint8_t *mask, int B, int T, int H, float *out, void *stream);
/* out (n,Cout) = x @ weight^T + bias (+ residual), Cin and Cout multiples of 64 up to 5120; out may be residual, not x.  Up to 768 input
 * channels: one launch, ascending k.  Beyond: the contraction is cut into ceil(Cin / 768) slices of equal length, each slice's sums go to
 * the workspace (ptx_txt_linear_workspace_bytes(n, Cin, Cout) bytes, 16-byte aligned; 0 without slices or out of range) and a second
 * launch adds the slices in ascending order, then the bias, then the residual. */
PTX_API size_t ptx_txt_linear_workspace_bytes(long n, int Cin, int Cout);
PTX_API int ptx_txt_linear(const float *x, long n, const float *weight, const float *bias, int Cin, int Cout, const float *residual,
                           float *out, void *workspace, size_t ws_bytes, void *stream);
/* out (n,C) = LayerNorm(x), the statistics as in ptx_txt_ln_linear; C: a multiple of 64 up to 1280.  One launch. */
PTX_API int ptx_txt_ln(const float *x, long n, int C, const float *weight, const float *bias, float eps, float *out, void *stream);

/* ------------------------------------------------------------------ the image backbone's convolutions (ABI 13, by addition)
 * The dense 2D convolutions of mmdet.ResNet (Bottleneck depths, every BatchNorm frozen) on NCHW float32 activations (csrc/conv2d.hip),
 * restated in numpy by image_backbone_host.py.  fp32 on the exact-fp32 matrix instruction (the stem: plain FMA), no float atomics, a
 * fixed k order: an image's bits depend neither on the batch size nor on its place in the batch; everything on `stream`, no host wait;
 * host checks (PTX_EINVAL with the numbers in the message) come before anything is enqueued.  The epilogue of all three, in the order of
 * ptx_sparse_conv3d: v * scale[co] + shift[co] (two roundings), + residual, ReLU; scale, shift, residual may be NULL.  The ReLU keeps a
 * NaN, and so does the stem's max-pool: a NaN pixel gives NaN in exactly the outputs whose receptive field holds it (torch's rule).
 *
 * The stem: out (N,C0,h2,w2) = max_pool2d(relu?(conv2d(xn, weight, stride 2, pad 3) * scale + shift), 3, stride 2, pad 1) in one launch,
 * h1 = (H-1)/2 + 1, h2 = (h1-1)/2 + 1 (likewise w); the half-resolution map is never written.  x (N,3,H,W): x_dtype 0 float32, 1 uint8.
 * xn = x, or with mean / std (3 floats each, on the device, both or neither) xn = ((float)x - mean[c]) / std[c], one float32 subtraction
 * and one correctly rounded float32 division, while the pixels are staged; the convolution's padding is zero AFTER that.  weight
 * (7*7*3, C0) = the (C0,3,7,7) kernel permuted to (ci, ky, kx, co) -- output channel contiguous.  C0: a multiple of 16 from 16 to 64;
 * H, W: 32 to 2048; N: 1 to 4096.  A work-group owns 6 x 16 pooled pixels. */
PTX_API int ptx_conv_stem(const void *x, int x_dtype, int N, int H, int W, const float *weight, int C0, const float *scale,
                          const float *shift, int relu, const float *mean, const float *std, float *out, void *stream);
/* out (N,Cout,Ho,Wo)[n,co,y,x] = epilogue(sum_ci weight[co,ci] x[n,ci,s y,s x]), s = stride 1 or 2, Ho = (H-1)/s + 1; weight (Cout,Cin);
 * residual (N,Cout,Ho,Wo).  Cin, Cout: multiples of 16 from 16 to 2048; H, W >= 1; N: 1 to 4096.  out may be residual, not x.  One
 * launch. */
PTX_API int ptx_conv1x1(const float *x, int N, int Cin, int H, int W, const float *weight, int Cout, int stride, const float *scale,
                        const float *shift, const float *residual, int relu, float *out, void *stream);
/* out (N,C,Ho,Wo) = epilogue(conv2d(x, w, stride s, pad 1)) as an implicit GEMM over k = (ky, kx, ci) (K = 9 C, no im2col buffer): weight
 * (C,3,3,C) = the (co,ci,ky,kx) kernel permuted to (co, ky, kx, ci) -- input channel contiguous.  C: a multiple of 16 from 16 to 512;
 * the rest as ptx_conv1x1.  One launch. */
PTX_API int ptx_conv3x3(const float *x, int N, int C, int H, int W, const float *weight, int stride, const float *scale,
                        const float *shift, const float *residual, int relu, float *out, void *stream);

/* ------------------------------------------------------------------ backward of ptx_conv1x1 / ptx_conv3x3 (ABI 13, by addition)
 * csrc/conv2d_bwd.hip, restated in numpy by image_backbone_grad_host.py.  With z the convolution before the epilogue, out =
 * relu((z * scale + shift) + residual) the forward's result and g = d loss / d out (N,Cout,Ho,Wo); every BatchNorm is frozen: scale and
 * shift take no gradient and there is no dbias.  Each of dresidual, dx, dweight is optional: NULL means it is not computed and its work
 * is not done.
 *   gz        (N,Cout,Ho,Wo) = g * [out > 0] * scale[co], each factor only where present (relu: 0 or 1, out is read only with relu;
 *             scale may be NULL); the mask is ptx_sparse_conv3d_bwd's: a NaN out passes nothing.  Scratch the call writes; required when
 *             (relu or scale) and (dx or dweight).  Without relu and scale the products read g itself and gz is not touched.
 *   dresidual (N,Cout,Ho,Wo) = g * [out > 0].  gz and dresidual come from one launch of their own (k_conv_epi_bwd), ahead of the others.
 *   dx        (N,Cin,H,W): dx[n,ci,y,x] = sum over every (ky, kx, co) whose output (oy, ox) = ((y + 1 - ky) / s, (x + 1 - kx) / s) exists
 *             (both numerators even at s = 2, inside the map; 1x1: (y / s, x / s)) of weight[co,ci,ky,kx] * gz[n,co,oy,ox], k = (ky, kx, co)
 *             ascending on the forward's tiles (16 rows x 256 pixels below 64 input channels, steps of 32 k; else 64 x 64, steps of 64 k;
 *             each step from zero, then added).  Every element is written: a pixel no output reads (odd rows and columns of a strided
 *             1x1) gets 0.0f; at stride 2 the structurally absent taps are multiplied by zero, the pixels are not split by parity.
 *             dx_accumulate = 1: the completed sum is added to what dx held, one rounding.  The weight is taken in the forward's layout
 *             and re-laid as (ci, ky, kx, co) into the workspace by a launch inside the call (k_conv_wt): no prepared transposed
 *             operand exists, so nothing has to be rebuilt after an optimizer step and every call pays for the re-layout.
 *   dweight   in the weight operand's layout, (Cout,Cin) or (co,ky,kx,ci): dweight[co,k] = sum over (n, oy, ox) of gz[n,co,oy,ox] *
 *             x[n,ci,s oy - 1 + ky,s ox - 1 + kx]; a tap outside the image is never read.  The flattened pixel index is cut into T =
 *             ceil(N Ho Wo / 64) steps of 64 and the steps are dealt evenly to S = ptx_conv_dweight_chunks(...) chunks (chunk c: steps
 *             [c T / S, (c + 1) T / S)); a chunk sums its steps in ascending order, each step's product from zero on the exact-fp32 matrix
 *             instruction and then added; the chunks' partials are added in ascending order (ptx_sparse_conv3d_bwd's slab sum).  S =
 *             min(ceil(1024 / tiles), ceil(T / 4), 256 MiB / the weight's bytes), at least 1, tiles = ceil(Cout / 64) ceil(K / 64): a function
 *             of the shapes only, which never falls when N grows.
 * No float atomics: two calls give the same bits.  Widths: multiples of 16, 16 to 2048 (1x1) / 16 to 512 (3x3); N, H, W, stride as the
 * forward takes them; x (N,Cin,H,W) is needed for dweight, weight for dx.  All float buffers and the workspace 16-byte aligned; no output
 * (gz, dresidual, dx, dweight, workspace) may overlap an input or another output.  workspace: ptx_conv_bwd_workspace_bytes(KS, ...) bytes
 * (KS 1 or 3, 3 with Cin = Cout; a function of the shapes only; 0: unsupported), needed for dx and, with S > 1, for dweight; a short one is
 * PTX_ENOSPACE.  Host checks (PTX_EINVAL with the numbers) come before anything is enqueued.  ptx_conv_dweight_chunks launches nothing
 * and answers PTX_EINVAL (negative) for unsupported shapes. */
PTX_API size_t ptx_conv_bwd_workspace_bytes(int KS, int N, int Cin, int Cout, int H, int W, int stride);
PTX_API int ptx_conv_dweight_chunks(int KS, int N, int Cin, int Cout, int H, int W, int stride);
PTX_API int ptx_conv1x1_bwd(const float *g, const float *out, const float *scale, int relu, const float *x, int N, int Cin, int H, int W,
                            const float *weight, int Cout, int stride, float *gz, float *dresidual, float *dx, int dx_accumulate,
                            float *dweight, void *workspace, size_t ws_bytes, void *stream);
PTX_API int ptx_conv3x3_bwd(const float *g, const float *out, const float *scale, int relu, const float *x, int N, int C, int H, int W,
                            const float *weight, int stride, float *gz, float *dresidual, float *dx, int dx_accumulate, float *dweight,
                            void *workspace, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PROXYT_H_ */
