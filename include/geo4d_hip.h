/* geo4d_hip.h — C ABI of libgeo4d_hip.so, the MI355X (gfx950 / CDNA4) kernel library behind the Geo4D
 * denoise + decode hot path.
 *
 * The reference (jzr99/Geo4D) has NO native boundary: its plug-in surface is the Python config registry
 * (utils/utils.py:27-42 instantiate_from_config) and below it only PyTorch ATen ops + xformers. This header is
 * therefore the boundary a reference maintainer would bind with ctypes: every entry point
 * replaces the ATen/xformers call(s) cited next to it. Conventions:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers owned by the caller (PyTorch allocator);
 *     the library never allocates, frees, synchronises or copies — every call only enqueues kernels on `stream`
 *     (a hipStream_t passed as void*), so every call is hipGraph-capturable;
 *   - activations are channels-last "tokens": row (b*T + t)*H*W + y*W + x, `ld*` = row pitch in ELEMENTS;
 *     dtype codes: 0 = f32 (exact parity mode, v_mfma_f32_32x32x2_f32), 1 = bf16, 2 = f16 (MFMA 32x32x16, fp32 acc);
 *     3 = bf16x3 (conv_gemm / attention only): operands are f32 in memory (4 bytes per element, `ld*` in elements) and
 *     are multiplied as bf16 hi + bf16 lo with three bf16 MFMAs per product (~16 mantissa bits at 1/3 of the bf16
 *     rate instead of 1/16 for f32 MFMA) — the mode that meets the 1e-3 parity bar; every other entry point takes 0 for it;
 *     4 = f16x2 (conv_gemm only, round 5; operand layout of round 6 = ABI 8): W PRE-SPLIT as [8 x f16 hi | 8 x f16 lo] per 8
 *     K-elements (4 bytes per element, `ldw` / `w_bs` in elements), A = PLAIN f16 rows (2 bytes per element, `lda` / `a_bs` in f16
 *     elements; a_split must be 2); the product is a.w_hi + a.w_lo — TWO f16 MFMAs: the activation carries 11 mantissa bits, the
 *     weight ~22. Used for the GEMMs of the "bf16x3m" mode whose A operand is a normalised branch activation (DESIGN.md section 3;
 *     tests/precision_sim.py); tile hints 0 or >= 22; f32 rows out, or (o_split = 2) plain f16 rows = the next dtype-4 launch's A;
 *   - every row pitch / base pointer must be 16-byte aligned (kernels move 16-byte chunks);
 *   - return 0 on success, negative errno-style code otherwise (-22 EINVAL, -95 ENOTSUP, -5 EIO = HIP launch
 *     error); geo4d_last_error() returns a thread-local message. Kernels never abort().
 *   - thread model: one host thread per device/stream; no global mutable state except per-kernel attribute caches.
 */
#ifndef GEO4D_HIP_H
#define GEO4D_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GEO4D_ABI_VERSION 9

/* Implicit-GEMM convolution / linear / batched GEMM:  out = epilogue(alpha * gather(A) . W^T)
 * replaces F.linear (attention.py:52-56,420,437), F.conv2d 3x3/1x1 stride 1|2 (openaimodel3d.py:154,179,65-67;
 * ae_modules.py:199-226), F.interpolate(nearest,2x)+conv (openaimodel3d.py:99-105; ae_modules.py:123-127),
 * F.conv3d (3,1,1) (openaimodel3d.py:257-266), torch.bmm (ae_modules.py:64,72), `+ emb_out[..., None, None]`
 * (openaimodel3d.py:222-230), residual adds, GEGLU (attention.py:415-422), SiLU. */
typedef struct geo4d_conv_gemm_t {
    const void* A;       /* input tokens [F*Hin*Win][lda]                              */
    const void* W;       /* packed weights [N][ldw], K = KT*KH*KW*Cin, tap-major        */
    void* O;             /* output [M][ldo] (or NCTHW when out_nchw)                    */
    const float* bias;   /* [N] (or [M] when bias_per_row), may be NULL                 */
    const float* rowbias;/* [M/rowbias_div][N] fp32 added per row group, may be NULL    */
    const void* R;       /* residual [M][ldr], dtype = out_dtype, may be NULL           */
    const void* zeros;   /* >= 16 zero bytes in device memory (source of padding taps)  */
    void* workspace;     /* fp32 scratch for split-K slabs (caller-owned, may be NULL)  */
    size_t workspace_bytes;
    long lda, ldw, ldo, ldr;
    long ldrb;           /* row pitch of rowbias in floats (0 = N)                      */
    long a_bs, w_bs, o_bs, r_bs; /* batch strides in elements (batched GEMM)            */
    int M, N, K, batch;
    int Cin;             /* channels per tap; multiple of 128 B worth of elements       */
    int T, Hin, Win, Hout, Wout;
    int KT, KH, KW, pt, ph, pw, stride, ups;
    int rowbias_div;
    int bias_per_row;
    int act;             /* 0 none, 1 SiLU, 2 GEGLU (packed pairs of 32 columns), 3 GELU (erf)   */
    int dtype;           /* A/W element type                                            */
    int out_dtype;       /* O/R element type                                            */
    int out_nchw;        /* 1: store O as [B][ldo][T][Hout*Wout] (ldo = channel count of the
                            destination tensor; O may point at a channel offset inside it) */
    int tile_hint;       /* 0 auto; 1..5 = 128x128, 128x64, 64x128, 64x64, 128x32 (4 waves, 2-stage ring);
                            8 waves, one tile per CU: 11 = 256x128, 13 = 256x256; 16 = 160x320 with 10 waves
                            (N = 320 layers: one tile per CU at M = 40960), 17 = 160x160 with 5 waves; no
                            GEGLU on 16 / 17. Second generation, bf16 / bf16x3 only (16x16x32 MFMA, register epilogue, persistent
                            workgroups; no NCTHW output, no gn_colsum): 22 = 256x256, 23 = 160x320 (8 waves, 80x80 wave
                            tiles), 25 = 128x128, 27 = 64x128, 28 = 64x64 (4 waves); GEGLU on 22, 25, 27. Third generation: the
                            same MFMA form and epilogue under a PHASED K loop (4 phases per slab, counted LDS-DMA waits, the
                            staging cursor two slabs ahead across tiles; 8 waves, one workgroup per CU): 71 = 192x256,
                            72 = 160x320, 73 = 256x128, 74 = 128x256; GEGLU on 71, 74; launches with an odd number or fewer
                            than 4 K slabs per tile, an uneven split-K or outputs that are not 4-element aligned run on
                            22 / 23 / 25 / 25 instead (same bits: every tile sums in the same order).
                            Others (incl. the hints retired in round 4: 12, 14, 21, 24, 26, 29, 31..39): -EINVAL */
    int split_k;         /* 0 auto (powers of two), 1 never, n >= 2: n-way split (needs workspace; tile hints >= 21 take any n) */
    int debug_ablate;    /* 0 in production. 2 (tests only, tile hints >= 22): launch 3 persistent workgroups whatever the problem size,
                            so that small test shapes walk the persistent tile loop; 16 + g (A/B runs): tile order with GROUP_M = g row-tiles
                            fastest instead of the column-fastest default (-9 % L2-miss fetch, -0.3 % frames/s: profiles/r05_tile_order.md);
                            + 64 (bit 6, combines with the values above; A/B runs and tests): 16-bit output rows keep the 8-byte register
                            epilogue instead of the 16-byte one (same bits, profiles/epilogue_wide.md) */
    float alpha;
    int a_split, w_split;/* dtype 3 (bf16x3): the operand is stored PRE-SPLIT, per 8 K-elements
                            [8 x bf16 hi | 8 x bf16 lo] (32 bytes, pack.py split_bf16) instead of 8 raw f32; dtype 4 (f16x2): w_split = 1
                            (f16 halves: pack.py split_f16) and a_split = 2 = A is plain f16 rows (geo4d_groupnorm_t.split_out = 2,
                            geo4d_layernorm_split fmt 2, o_split = 2 of a previous dtype-4 launch) */
    int o_split;         /* 2 (dtype 4 only; out_dtype F32, no residual, no split-K): O is written as PLAIN f16 rows (ldo / o_bs in f16 elements,
                            stored columns % 8 == 0, 16-byte aligned rows), values clamped to the finite f16 range, NaN kept - the A operand of a following
                            dtype-4 launch (GEGLU -> FF-out). 1: dtype 3 (bf16x3), a_split and w_split set, out_dtype F32: O is written in the pre-split operand
                            format ([8 x bf16 hi | 8 x bf16 lo] per 8 output columns; ldo / o_bs still count columns) - the producer
                            side of a_split (GEGLU -> FF-out chain; q | k and V^T of the spatial attention, geo4d_attention_t.qkv_split).
                            Stored columns % 8 == 0, ldo % 8 == 0, 32-byte aligned rows, no split-K, any epilogue incl. residual;
                            served by the second- / third-generation tiles (first-generation hints are re-routed) */
    float* gn_colsum;    /* optional [M/rows][N][2] fp32 (rows = geo4d_conv_gemm_colsum_rows(p): 32 for the first generation): per row block and output column, (sum, sum of squares) of the values this
                            launch stores - the statistics pass of the GroupNorm that consumes O, produced for free by the epilogue
                            (geo4d_groupnorm_t.colsum). Needs M % 32 == 0, N % 8 == 0, row-major 16-byte aligned output, batch 1,
                            no GEGLU; no split-K on the first generation. Round 6: a split-K launch of tile hints >= 22 emits them from its
                            reduce launch, per 32 rows (N % 64 == 0) or, where a frame's Hout x Wout rows are a multiple of 8 but not of 32, per
                            8 rows (N % 256 == 0): geo4d_conv_gemm_colsum_rows says which. */
    unsigned long long* sat_count; /* optional DEBUG counter in device memory (NULL in production): o_split = 2 launches add the number of
                            (wave, store) lanes whose value lay beyond the finite f16 range and was clamped. Tests assert it stays 0. */
} geo4d_conv_gemm_t;
int geo4d_conv_gemm(const geo4d_conv_gemm_t* p, void* stream);
/* What a launch of `*p` becomes: the answer of the host-side planner (csrc/gemm_plan.h) that geo4d_conv_gemm itself launches from. */
typedef struct geo4d_conv_gemm_plan_t {
    int tile_hint;       /* the tile that runs, after defaults, redirects and fall-backs: a launch with it set explicitly runs the same kernel */
    int generation;      /* its kernel generation: 1 (hints below 21), 2 (21..70) or 3 (from 71)                                           */
    int bm, bn, wm, wn;  /* workgroup tile bm x bn on wm x wn waves                                                                        */
    int splits;          /* K slices (gridDim.z); > 1 is followed by the reduce launch                                                     */
    int hot;             /* operand-layout variant compiled in (4-byte types): 0 generic, 1 raw A x split W, 2 split A x split W           */
    int osplit;          /* 1: the epilogue writes a producer format (o_split 1 / 2)                                                       */
    int colsum_rows;     /* rows per gn_colsum entry this launch emits (would emit, where gn_colsum is NULL); 0 = it cannot                */
} geo4d_conv_gemm_plan_t;
/* pure host function: validates `p` exactly as geo4d_conv_gemm does (gn_colsum included: a launch that cannot emit the sums it is asked
   for is refused) and says what it would launch; the launch's own return code, geo4d_last_error() set on refusal */
int geo4d_conv_gemm_plan(const geo4d_conv_gemm_t* p, geo4d_conv_gemm_plan_t* plan);
/* One row of the planner's tile table per tile hint that exists. */
typedef struct geo4d_conv_gemm_tile_t {
    int tile_hint, generation, bm, bn, wm, wn;
    int geglu;           /* 1: the tile takes act = 2 (wave tiles a multiple of 64 columns wide)                                           */
} geo4d_conv_gemm_tile_t;
/* pure host function: writes the first `cap` rows of the tile table to `out` (may be NULL with cap 0) and returns how many there are */
int geo4d_conv_gemm_tiles(geo4d_conv_gemm_tile_t* out, int cap);
/* The colsum_rows of the same plan WITHOUT the descriptor checks (the query older than geo4d_conv_gemm_plan, kept for its callers): rows of
   the output that ONE gn_colsum entry of the launch `*p` covers (tile_hint / split_k as they will be launched, the gn_colsum field itself ignored): 32 for
   the first-generation tiles, the wave tile's rows (32..128) for tile hints >= 21 without split-K, 32 or 8 for their split-K launches (the
   reduce launch sums them); 0 = this launch cannot emit the sums, or the planner refuses it. gn_colsum then has [M / rows][N][2] floats. */
int geo4d_conv_gemm_colsum_rows(const geo4d_conv_gemm_t* p);
/* Nearest-2x upsampling + 3x3 convolution (pad 1) in its sub-pixel form: per output parity (py, px) the operation is a 2x2 convolution on
   the SOURCE grid [F, H, W] whose weights are sums of the 3x3 ones (geo4d_amd/pack.py fold_up2: rows {y - 1: W[-1], y: W[0] + W[1]} for
   py = 0, {y: W[-1] + W[0], y + 1: W[1]} for py = 1, columns alike) - 4 / 9 of the multiplications of the ups = 2 gather, same passes.
   `*p` describes that 2x2 convolution: ups 1, KH = KW = 2, stride 1, Hout = Hin = H, Wout = Win = src_w = W, M = F H W, K = 4 Cin, and O
   the [F, 2H, 2W] token grid: row m = (f, y, x) is stored at row 4 W (m div W) + 2 (m mod W) + py 2W + px.
   phase 0..3 = 2 py + px: one launch per phase, batch 1, ph = 1 - py, pw = 1 - px, W that phase's weight;
   phase -1: ONE launch, the phase is the batch index (batch 4, a_bs = o_bs = 0, w_bs = the stride between the phase weights; ph / pw are
   set per phase by the kernel).
   dtype 3 (bf16x3) against a pre-split weight (raw or pre-split activations), tile hints 22, 23, 25, 71, 72, plain f32 rows with a column
   bias: no activation, residual, row biases, split-K, o_split or NCTHW output - everything else is refused (csrc/gemm_plan.h resolve_up2).
   gn_colsum: [M / rows][4][N][2] - the entries of the four phases interleave, so that the buffer reads as the [4 M / rows][N][2] sums of O
   with each frame's entries contiguous; needs H W % rows == 0 (rows = the plan's colsum_rows). */
int geo4d_conv_gemm_up2(const geo4d_conv_gemm_t* p, int src_w, int phase, void* stream);
/* pure host function: what geo4d_conv_gemm_up2 would launch, or its refusal (the launch's own return code and message) */
int geo4d_conv_gemm_up2_plan(const geo4d_conv_gemm_t* p, int src_w, int phase, geo4d_conv_gemm_plan_t* plan);

/* GroupNorm(groups) [+SiLU] over tokens [F][HW][C]; statistics per (F / frames_per_stat, group) in fp32.
 * replaces nn.GroupNorm / GroupNormSpecific + nn.SiLU (basics.py:76-87; openaimodel3d.py:151-153,174-176,256-266;
 * attention.py:265,331; ae_modules.py:10-16). */
typedef struct geo4d_groupnorm_t {
    const void* x; void* y;
    const float* gamma; const float* beta;
    void* workspace; size_t workspace_bytes;
    long ldx, ldy;
    int F, HW, C, groups, frames_per_stat;
    int act;             /* 0 none, 1 SiLU / swish                                       */
    int dtype;
    float eps;
    const float* colsum; /* optional: [F*HW/colsum_rows][C][2] column sums written by the producing geo4d_conv_gemm (gn_colsum); when
                            given the pass over x that computes the statistics is skipped */
    int split_out;       /* producers of GEMM operands (dtype F32 only, C % 8 == 0): 1: y is written in the PRE-SPLIT operand format of
                            geo4d_conv_gemm_t.a_split, per 8 channels [8 x bf16 hi | 8 x bf16 lo] (bf16x3 consumers; ldy counts channels = 4-byte
                            units); 2: y = PLAIN f16 rows (ldy in f16 elements), values clamped to the finite f16 range, NaN kept (dtype-4 consumers) */
    int colsum_rows;     /* rows per `colsum` entry (what geo4d_conv_gemm_colsum_rows returned for the producing launch); 0 = 32;
                            (frames_per_stat x HW) % colsum_rows == 0 */
    unsigned long long* sat_count; /* optional DEBUG counter (see geo4d_conv_gemm_t.sat_count) of the split_out = 2 clamp; NULL in production */
} geo4d_groupnorm_t;
size_t geo4d_groupnorm_workspace(int F, int HW, int groups, int frames_per_stat);
int geo4d_groupnorm(const geo4d_groupnorm_t* p, void* stream);

/* The same GroupNorm with up to TWO sources of column sums (a channel concatenation whose halves were written by two GEMM launches,
 * each with its own rows per entry) and a choice of launch sequence. `base.colsum` / `base.colsum_rows` are ignored here: the sums
 * come from `src`. geo4d_groupnorm(p) == geo4d_groupnorm2 with one source {p->colsum, p->colsum_rows, 0, C} (or none) and path 0. */
typedef struct geo4d_groupnorm_src_t {
    const float* colsum; /* [F*HW/rows][channels][2] (sum, sum of squares), as geo4d_conv_gemm_t.gn_colsum of the producing launch        */
    int rows;            /* rows per entry; (frames_per_stat x HW) % rows == 0                                                            */
    int c0, channels;    /* the columns [c0, c0 + channels) of x this source covers: the sources tile [0, C) in order                     */
} geo4d_groupnorm_src_t;
typedef struct geo4d_groupnorm2_t {
    geo4d_groupnorm_t base;
    geo4d_groupnorm_src_t src[2];
    int nsrc;            /* 0 (statistics pass over x), 1 or 2                                                                            */
    int path;            /* 0 = the library decides (geo4d_groupnorm_plan); GEO4D_GN_PATH_* forces one (A/B, tests, tools/norm_bench.py)  */
    float fuse_fraction; /* 0 = default (1/8, else 1/4, while the launch re-reads <= 12 MiB of sums); else the largest (sum bytes :
                            payload bytes) per workgroup at which path 0 still fuses, with no bound on the re-read sums (sweeps)          */
    int min_workgroups;  /* 0 = default; else the fewest workgroups path 0 lets a fused launch have                                       */
} geo4d_groupnorm2_t;
enum {
    GEO4D_GN_PATH_PARTIAL = 1,  /* gn_partial + gn_finalize + gn_apply: what runs without sums                                            */
    GEO4D_GN_PATH_COLS = 2,     /* gn_finalize_cols + gn_apply (one full-width source only; else PARTIAL): the two-launch sequence; path 0
                                   keeps it for per-frame statistics whose sums are too large to fuse                                     */
    GEO4D_GN_PATH_FUSED = 3,    /* ONE launch: every workgroup of gn_apply reduces its statistic's sums in its prologue                  */
    GEO4D_GN_PATH_SLICED = 4    /* gn_slice_sums (stat_slices workgroups per (statistic, group)) + gn_apply combining the partials       */
};
typedef struct geo4d_groupnorm_plan_t {
    int path;            /* GEO4D_GN_PATH_* that a launch with these arguments runs                                                       */
    int launches;
    int rows_per_wg;     /* rows of one frame per workgroup of the apply launch, and chunks per frame                                     */
    int nchunk;
    int channel_slices;  /* FUSED: workgroups across the channels (each a whole number of groups), so that fewer, taller workgroups
                            read fewer sums each while the launch keeps its workgroup count                                              */
    int stat_slices;     /* SLICED: partial sums per (statistic, group)                                                                   */
    size_t workspace_bytes; /* what the chosen path writes; <= geo4d_groupnorm_workspace(F, HW, groups, frames_per_stat)                  */
} geo4d_groupnorm_plan_t;
/* pure host function: validates `p` exactly as geo4d_groupnorm2 does (except the workspace size) and says what it would launch */
int geo4d_groupnorm_plan(const geo4d_groupnorm2_t* p, geo4d_groupnorm_plan_t* plan);
int geo4d_groupnorm2(const geo4d_groupnorm2_t* p, void* stream);

/* LayerNorm over the last dim; replaces nn.LayerNorm (attention.py:225-227). */
int geo4d_layernorm(const void* x, long ldx, void* y, long ldy, int M, int C, float eps, const float* gamma,
                    const float* beta, int dtype, void* stream);

/* the same for an f32 x, writing y in a GEMM-operand format (geo4d_groupnorm_t.split_out: fmt 1 = pre-split bf16 hi | lo, ldy in
 * 4-byte units; fmt 2 = plain f16 rows, ldy in f16 elements, clamped, `sat_count` = optional debug counter of the clamp or NULL); C % 8 == 0. */
int geo4d_layernorm_split(const void* x, long ldx, void* y, long ldy, int M, int C, float eps, const float* gamma,
                          const float* beta, int fmt, unsigned long long* sat_count, void* stream);

/* y = softmax(scale * x) per row, x fp32; replaces F.softmax in the VAE AttnBlock (ae_modules.py:66-68). */
int geo4d_softmax_rows(const float* x, long ldx, void* y, long ldy, long rows, int cols, float scale, int out_dtype,
                       void* stream);
/* the same with a causal mask: row r attends to columns <= r % causal_period (the attn_mask of the OpenCLIP text transformer,
 * condition.py:217-221; rows of several (batch, head) score matrices of `causal_period` rows each stacked). */
int geo4d_softmax_rows_causal(const float* x, long ldx, void* y, long ldy, long rows, int cols, float scale, int out_dtype,
                              int causal_period, void* stream);

/* Fused multi-head attention, d_head = 64, no mask, up to two key/value sets with independent softmaxes whose
 * outputs are summed. q rows: b*Nq + i, head h at columns [64h, 64h+64). K rows of set s: (b / kv_div[s])*Nk[s] + j.
 * V is passed TRANSPOSED: vt[s] + (b / kv_div[s]) * vt_bs[s] + (64h + d) * ldvt[s] + j  (row = channel, column = key;
 * the row must be readable — zero or finite — up to the next multiple of 16 bytes past Nk). `zeros`: >= 16 zero bytes.
 * replaces CrossAttention.forward / efficient_forward = xformers.ops.memory_efficient_attention
 * (attention.py:81-144, 146-209). */
typedef struct geo4d_attention_t {
    const void* q; void* o;
    const void* k[2]; const void* vt[2];
    const void* zeros;
    long ldq, ldo, ldk[2], ldvt[2], vt_bs[2];
    int Nk[2], kv_div[2];
    int B, H, Nq, nseg, head_dim, dtype;
    float scale;
    int split_out;       /* 4-byte storage only (dtype F32 or BF16X3 - the bf16x3 mode stores its activations as f32): o is written in the pre-split operand format of geo4d_conv_gemm_t.a_split (ldo still
                            counts channels) - the to_out projection consumes it without splitting again */
    int variant;         /* 0 = default; A/B builds of the same math: 1 = 128 query rows per workgroup, 2 = the same compiled for
                            4 waves per SIMD (16-bit types), 3 = 256 rows per workgroup, two query blocks per wave (nseg == 1),
                            4 = 256 rows per workgroup with the two blocks' phases skewed so every softmax has the other block's MFMAs
                            beside it (nseg == 1; bf16 / f16, and bf16x3 with qkv_split at one wave per SIMD), 5 = the bf16x3 form of 4
                            at two waves per SIMD */
    int qkv_split;       /* dtype 3 (bf16x3), nseg == 1 only: q, k[0] and vt[0] are stored in the PRE-SPLIT operand format (written by
                            geo4d_conv_gemm_t.o_split projections): per 8 elements of a row [8 x bf16 hi | 8 x bf16 lo]; ld* / vt_bs still
                            count 4-byte elements and must be multiples of 8, bases 32-byte aligned, Nk % 8 == 0. Same results, bit
                            for bit, as the raw-f32 inputs (the split is the same arithmetic, done once by the producer). */
} geo4d_attention_t;
typedef struct geo4d_attention_plan_t {
    int kernel;          /* 1 = flash_attn_kernel, 2 = flash_attn2_kernel (skewed query blocks)                                           */
    int nseg;            /* key/value sets the instantiation is compiled for                                                              */
    int qb;              /* 32-row query blocks per wave                                                                                  */
    int occ;             /* waves per SIMD the instantiation is compiled for                                                              */
    int ps;              /* the instantiation reads pre-split q / k / vt (qkv_split)                                                      */
    int rows_per_wg;     /* query rows per workgroup: 128 or 256                                                                          */
    unsigned grid[3];    /* {ceil(Nq / rows_per_wg), H, B} workgroups of 256 threads                                                      */
    int variant;         /* the `variant` that runs, after defaults and fall-backs: a launch with it set explicitly runs the same kernel  */
} geo4d_attention_plan_t;
/* pure host function: validates `p` exactly as geo4d_attention does and says what it would launch */
int geo4d_attention_plan(const geo4d_attention_t* p, geo4d_attention_plan_t* plan);
int geo4d_attention(const geo4d_attention_t* p, void* stream);

/* Self-attention over T <= 16 frames for every (batch, pixel, head); tokens stay frame-major [B*T][HW][C].
 * replaces the einsum/softmax path of CrossAttention inside TemporalTransformer (attention.py:101-125, 365-412). */
int geo4d_temporal_attention(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo,
                             int B, int T, int HW, int H, int head_dim, float scale, int dtype, void* stream);
/* the same with `split_out` (dtype GEO4D_F32 only = the storage type of the bf16x3 mode; dtype 3 is NOT accepted here): o in the
 * pre-split operand format, see geo4d_attention_t.split_out */
int geo4d_temporal_attention2(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo,
                              int B, int T, int HW, int H, int head_dim, float scale, int dtype, int split_out, void* stream);

/* [B,C0,T,H,W] (+ [B,C1,T,H,W]) fp32 -> tokens [(b t) hw][Cpad] (zero padded);
 * replaces torch.cat([x] + c_concat, 1) + rearrange (ddpm3d.py:2540-2544; openaimodel3d.py:588). */
int geo4d_tokens_from_ncthw(const float* src0, int C0, const float* src1, int C1, void* out, int Cpad, int B, int T, int HW,
                            int dtype, void* stream);

/* out[m] = [a[m] | b[m]]; replaces torch.cat([h, hs.pop()], dim=1) (openaimodel3d.py:624-626). */
int geo4d_concat_channels(const void* a, long lda, int Ca, const void* b, long ldb, int Cb, void* out, long ldo, long M,
                          int dtype, void* stream);

/* y = f16(x) row by row: the A operand of a dtype-4 (two-pass f16) geo4d_conv_gemm launch made from an f32 tensor that has no normalising
 * producer in front of it - the VAE decoder's residual stream in front of its Upsample convolutions (ae_modules.py:111-127), bf16x3m class
 * "vaeup". Values clamped to the finite f16 range, NaN kept; `sat_count` = optional debug counter of the clamp (NULL in production). C % 8 == 0. */
int geo4d_cast_rows_f16(const float* x, long ldx, void* y, long ldy, long M, int C, unsigned long long* sat_count, void* stream);

/* y = x in the PRE-SPLIT bf16x3 operand format (geo4d_conv_gemm_t.a_split = 1: per 8 elements [8 x bf16 hi | 8 x bf16 lo]; ldy counts 4-byte units like
 * ldx): what the GEMM's in-register split computes per fragment and K slab, done ONCE - for the long-K launches whose A operand is a residual stream
 * (the Upsample convolutions of the U-Net and of the VAE decoder: every input element is gathered 9 x 4 times). Same arithmetic, same bits. C % 8 == 0. */
int geo4d_split_rows_bf16(const float* x, long ldx, void* y, long ldy, long M, int C, void* stream);

/* out[b] = [cos(t_b * f) | sin(t_b * f)]; replaces timestep_embedding (utils_diffusion.py:8-28). */
int geo4d_timestep_embedding(const long* t, const float* freqs, float* out, int B, int dim, void* stream);

/* out = act_out(act_in(x) . W^T + bias) + add, all fp32, M small; replaces time_embed / fps_embedding /
 * ResBlock.emb_layers (openaimodel3d.py:367-384, 166-172, 222). */
int geo4d_linear_small(const float* x, long ldx, const float* w, long ldw, const float* bias, const float* add, long ldadd,
                       float* out, long ldo, int M, int N, int K, int act_in, int act_out, void* stream);

/* In-place DDIM update of x with v-prediction and dynamic rescale; coefficients are read from
 * coef[*step_index] (6 floats per step) so one captured hipGraph replays for every step.
 * replaces DDIMSampler.p_sample_ddim arithmetic (ddim.py:232-277) + DDPM.predict_* (ddpm3d.py:278-290). */
int geo4d_ddim_step(float* x, const float* v, const float* noise, float* pred_x0, const float* coef, const int* step_index,
                    long n, void* stream);
/* Counter-based Gaussian noise (Philox4x32-10, Salmon et al. SC'11; DESIGN.md section 15, restated in numpy by geo4d_amd/noise.py).
 * The value of element i of sample b is a pure function of (seeds[b], step, stream_id, draw, i): key = (seed low word, seed high word),
 * counter = (i / 4, step, stream_id, draw), element i takes output word i % 4; words (0, 1) and (2, 3) are two Box-Muller pairs with
 * u1 = ((w_a >> 8) + 1) 2^-24, u2 = (w_b >> 8) 2^-24, even word: sqrt(-2 ln u1) cos(2 pi u2), odd word: sqrt(-2 ln u1) sin(2 pi u2);
 * never NaN / Inf, |z| <= 5.768. stream_id: 0 = initial noise x_T, 1 = DDIM step noise (2 reserved). seeds: int64 [B] in DEVICE memory;
 * step = *step_index when step_index != NULL (device int, so a captured launch follows the step counter), else step_value.
 * kind 0: out = fp32 [B][n_per_sample] normals * scale; kind 1: out = uint32 [B][n_per_sample] raw words (scale ignored).
 * n_per_sample <= 2^34. Rows that are whole 16-byte quads (n_per_sample % 4 == 0, aligned base) take one Philox call per quad. */
int geo4d_philox_fill(void* out, int kind, const long* seeds, int B, long n_per_sample, const int* step_index, int step_value,
                      int stream_id, int draw, float scale, void* stream);
/* The DDIM update above on x / v / pred_x0 = [B][n_per_sample] with noise[b][i] = the stream-1 normal of (seeds[b], *step_index, i, draw)
 * * noise_scale made in registers: same bits as the fill (kind 0, scale = noise_scale) into a buffer passed as `noise` to the update above.
 * The stochastic (eta > 0) step then holds nothing host-dependent: capturable, and a sample's noise does not depend on its batch. */
int geo4d_ddim_step_rng(float* x, const float* v, float* pred_x0, const float* coef, const int* step_index, const long* seeds, int B,
                        long n_per_sample, int draw, float noise_scale, void* stream);
/* Classifier-free guidance on fp32 [B][n] U-Net outputs:
 *   out = e_u + cfg_img (e_i - e_u) + scale (e_c - e_i)          (e_i == NULL: out = e_u + scale (e_c - e_u))
 *   guidance_rescale > 0: out = r * out * std(e_c)/std(out) + (1 - r) * out, unbiased std per batch sample over the n other elements
 * replaces the combination in DDIMSampler.p_sample_ddim (ddim.py:216-229; 3-way: ddim_multiplecond.py:229-236) and
 * rescale_noise_cfg (utils_diffusion.py:147-158). workspace: geo4d_cfg_combine_workspace(B) bytes, 8-byte aligned. */
size_t geo4d_cfg_combine_workspace(int B);
int geo4d_cfg_combine(const float* e_c, const float* e_u, const float* e_i, float* out, int B, long n, float scale, float cfg_img,
                      float guidance_rescale, void* workspace, size_t workspace_bytes, void* stream);
/* out[(b n)][:] = table[tokens[b][n]][:] + pos[n][:]; replaces token_embedding(text) + positional_embedding of the OpenCLIP text
 * tower (condition.py:212-214). table [vocab][width], pos [n_ctx][width] fp32; rows = B * n_ctx; out-of-range ids read row 0. */
int geo4d_embed_tokens(const long* tokens, const float* table, const float* pos, void* out, long ldo, long rows, int n_ctx,
                       int width, int vocab, int dtype, void* stream);
int geo4d_advance_index(int* idx, int delta, void* stream);
/* ts[b] = table[*idx] for b < B: the per-step `ts = torch.full((b,), step)` of ddim.py:170, read from a device table so
 * the captured step graph is step-independent. */
int geo4d_gather_timestep(const int* idx, const long* table, long* ts, int B, void* stream);

/* Plücker ray map -> camera-to-world matrices of one window. replaces raymap_to_camera_matrix
 * (scripts/evaluation/test_geo4d.py:539-557) -> cameras_from_plucker / rays_to_cameras (utils/rays.py:387-433, 301-368) ->
 * intersect_skew_lines_high_dim (utils/normalize.py:25-51) + compute_optimal_rotation_alignment (utils/rays.py:579-595), which the
 * reference runs on the host. ray / moment: fp32 planes [3][T][H][W] addressed as base + c*channel_stride + t*frame_stride + y*W + x
 * (so they can be channel views of the decoded [B,11,T,H,W] tensor); frame 0 is the reference frame; the maps are centre-cropped to
 * min(H,W)^2 like the reference. P_c2w: [T][4][4] fp32 row-major. workspace: geo4d_plucker_cameras_workspace bytes, 8-byte aligned. */
size_t geo4d_plucker_cameras_workspace(int T, int H, int W);
int geo4d_plucker_cameras(const float* ray, const float* moment, long channel_stride, long frame_stride, int T, int H, int W,
                          void* workspace, size_t workspace_bytes, float* P_c2w, void* stream);

/* Multi-window global alignment, one iteration's residual + gradients. replaces the autograd forward /
 * backward of LightPointCloudGroupOptimizer.forward's point-map term (dust3r/cloud_opt/optimizer_group.py:440-455 with
 * depth_to_pts3d :407-417 and l1_dist commons.py:86-87). A "slot" is one (window, frame) prediction; image i owns the slots
 * slot_idx[slot_ptr[i] .. slot_ptr[i+1]).  loss = inv_area * sum min(conf, conf_clamp) * | X_i - (sR_g P + st_g) |.
 *   pred [n_slots][H*W][3], conf [n_slots][H*W], logdepth / grad_logdepth [n_imgs][H*W]          (fp32, device)
 *   cams [n_imgs][16] = R (9, row-major) | t (3) | focal | ppx | ppy | 0      slot_trf [n_slots][12] = sR (9) | st (3)
 *   img_sums [n_imgs][14] = dL/dR (9) | dL/dt (3) | dL/dfocal | loss share
 *   slot_sums [n_slots][14] = dL/d(sR) (9) | dL/d(st) (3) | dL/ds_depth, dL/dt_depth (inverse-depth term; 0 when off), in CSR order
 * Inverse-depth term (optimizer_group.py:470-494), fused into the same pass when invdepth != NULL:
 *   loss += depth_weight * sum_{slot, pixel: q > 0.05} accepted_g * | 1 / (exp(logdepth) + 1e-6) - (s_g q + t_g) |
 *   invdepth [n_slots][H*W] = q, slot_st [n_slots][3] = (s_g, t_g, accepted_g in {0, 1}); the reference's factor 2 / total area is depth_weight.
 * workspace: geo4d_align_workspace bytes. Deterministic (fixed-order reductions). */
typedef struct geo4d_align_t {
    const float* pred; const float* conf; const float* logdepth; const float* cams; const float* slot_trf;
    const int* slot_ptr; const int* slot_idx;
    float* grad_logdepth; float* img_sums; float* slot_sums;
    void* workspace; size_t workspace_bytes;
    float* img_part; float* slot_part;   /* set by the library (views of workspace) */
    const float* invdepth; const float* slot_st;   /* inverse-depth term (NULL: off), see below */
    int n_imgs, n_slots, H, W, chunk_pixels, max_slots_per_image;
    float conf_clamp, inv_area, depth_weight;
} geo4d_align_t;
size_t geo4d_align_workspace(int n_imgs, int n_slots, int H, int W, int chunk_pixels);
int geo4d_align_residual(const geo4d_align_t* p, void* stream);
/* Principal-point form (optimizer_group.py:67-68, 203-211: im_pp per image, principal point = (W/2, H/2) + 10 im_pp, optimize_pp).
 *   geo4d_align_set_pp       cams[i][13..14] = (ppx, ppy) + 10 im_pp[i]  (im_pp [n_imgs][2]); run it after geo4d_align_refresh, which
 *                            writes the scalar centre there. geo4d_align_residual reads whatever cams holds, so a preset (frozen)
 *                            principal point needs only this launch.
 *   geo4d_align_residual_pp  geo4d_align_residual + pp_sums [n_imgs][2] = (dL/dppx, dL/dppy) = -sum_px (c0, c1) d / f with c = R^T g the
 *                            camera-frame gradient; the two sums ride through the same fixed-order block and chunk reductions as the 14
 *                            image sums (deterministic), every other output equals geo4d_align_residual's bit for bit. Dispatches to the
 *                            slot-outer kernel ONLY: chunk_pixels in {256, 1024, 2048, 4096}, anything else is -ENOTSUP (and
 *                            GEO4D_ALIGN_KERNEL=1 is not consulted). workspace: geo4d_align_pp_workspace bytes.
 *   geo4d_align_pp_grads     grad_im_pp [n_imgs][2] = 10 pp_sums. */
size_t geo4d_align_pp_workspace(int n_imgs, int n_slots, int H, int W, int chunk_pixels);
int geo4d_align_residual_pp(const geo4d_align_t* p, float* pp_sums, void* stream);
int geo4d_align_set_pp(float* cams, const float* im_pp, int n_imgs, float ppx, float ppy, void* stream);
int geo4d_align_pp_grads(const float* pp_sums, float* grad_im_pp, int n_imgs, void* stream);
/* One torch.optim.Adam step on a flat fp32 tensor (no weight decay / amsgrad); `step` counts from 1.
 * replaces optimizer.step() of global_alignment_iter (dust3r/cloud_opt/base_opt_group.py:596-626) for the depth maps. */
int geo4d_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                    float eps, int step, void* stream);
/* The same with {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read from device memory (3 floats), so a captured hipGraph of one whole
 * alignment iteration can be replayed while the schedule advances on the device. */
int geo4d_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, const float* hyper, float beta1,
                        float beta2, float eps, void* stream);

/* The parameter side of one alignment iteration (round 3; base_opt_group.py:262-327 parameterisation, optimizer_group.py:529-541
 * relative_pose_loss): geo4d_align_refresh writes the residual kernel's inputs from the parameters - cams [n_imgs][16] =
 * (R row-major | t | f | ppx | ppy | 0) with R = rotation of the NORMALISED XYZW quaternion im_poses[i][0:4], t = signed_expm1 of
 * im_poses[i][4:7], f = exp(im_focals / focal_break); slot_trf [n_slots][12] = (s_g R_g | s_g t_g) of the slot's window g = slot /
 * slots_per_group with s_g = exp(pw_poses[g][7] + (norm_pw_scale ? log base_scale - mean_g pw_poses[g][7] : 0)).
 * geo4d_align_small_grads turns the residual kernel's gradient sums (img_sums [n_imgs][14]; slot_sums [n_listed_slots][14] in the CSR
 * order of slot_idx, listed per window by group_ptr / group_entries) into loss[0] = sum_i img_sums[i][13] + smooth_weight * sum_i
 * relative_pose_loss(cam_i, cam_i+1) and the gradients of im_poses [n_imgs][7], im_focals [n_focals] (1 = shared), pw_poses
 * [n_groups][8] and, when given, s_depth / t_depth [n_groups]. One workgroup, fixed-order sums, fp64 inside (several of the sums cancel).
 * replaces loss.backward() through the tiny parameter tensors (round 2: ~450 autograd launches per iteration). */
typedef struct geo4d_align_small_t {
    const float* im_poses; const float* im_focals; const float* pw_poses;
    float* cams; float* slot_trf;
    const float* img_sums; const float* slot_sums;
    const int* group_ptr; const int* group_entries;   /* window g owns CSR entries group_entries[group_ptr[g] .. group_ptr[g + 1]) (ascending) */
    double* group_sums; double* scale_terms;   /* scratch: [n_groups][14] and [n_groups] fp64 */
    float* grad_im_poses; float* grad_im_focals; float* grad_pw_poses; float* grad_s_depth; float* grad_t_depth; float* loss;
    /* inverse-depth term (all NULL: off): geo4d_align_refresh also writes slot_st [n_slots][3] = (s_depth[g], t_depth[g], depth_ok[g]) */
    float* slot_st; const float* s_depth; const float* t_depth; const float* depth_ok;
    /* trajectory term (traj NULL: off; optimizer_group.py:496-512): traj [n_slots][4][4] = every window's predicted camera-to-world
     * matrices, traj_align [n_groups][8] = traj_align_poses, traj_valid [n_groups] (0 / 1), slot_img [n_slots] = image of a slot,
     * img_slot_ptr / img_slot_idx = CSR of ALL slots per image; loss += traj_weight * sum relative_pose_loss(T_g [R_k | e^l t_k], cam_i);
     * grad_traj [n_groups][8] receives d/d traj_align_poses (zero rows for invalid windows); the camera side is added to grad_im_poses */
    const float* traj; const float* traj_align; const int* traj_valid; const int* slot_img; const int* img_slot_ptr; const int* img_slot_idx;
    float* grad_traj;
    int n_imgs, n_groups, n_slots, slots_per_group, n_listed_slots, n_focals, norm_pw_scale;
    float focal_break, base_scale, ppx, ppy, smooth_weight, translation_weight, traj_weight;
} geo4d_align_small_t;
int geo4d_align_refresh(const geo4d_align_small_t* p, void* stream);
int geo4d_align_small_grads(const geo4d_align_small_t* p, void* stream);

/* Start-up of the inverse-depth term (LightPointCloudGroupOptimizer._set_st_depth, optimizer_group.py:333-372, which calls
 * dust3r/depth_eval.py depth_evaluation(align_with_lad2=True) :147-330 per window). All arrays fp32 on the device, windows
 * contiguous: q / target / conf are [G][n], n = S * H * W.
 *   geo4d_lad_target: target[slot][px] = 1 / (exp(logdepth[slot_img[slot]][px]) + 1e-6)                     (:336-337)
 *   geo4d_lower_median: out[r] = torch.median(x[r]) (the LOWER median), bit-exact, by radix select; workspace rows * 260 * 4 bytes
 *   geo4d_lad_fit: (s, t)[g] minimising sum | s q + t - target | by torch.optim.Adam's arithmetic (default betas), started at
 *     s = median(target) / median(q), t = 0; a window stops when its loss repeats within tol (depth_eval.py:112-145, 218-221).
 *     active (NULL = all): windows with 0 are left at their start values. st_out [G][2]; info_out (may be NULL) [G][2] = (steps, last loss).
 *   geo4d_lad_delta: counts[g] = {#(max(a/target, target/a) < 1.25), #mask}, a = max(s q + t, 1e-5), mask = min(conf, conf_clamp) >
 *     conf_thr and q > q_thr (:297-301 under _set_st_depth's custom mask :340-342). */
size_t geo4d_lad_workspace(int G, long n);
int geo4d_lad_target(const float* logdepth, const int* slot_img, float* target, int n_slots, int HW, void* stream);
int geo4d_lower_median(const float* x, int rows, long n, float* out, void* workspace, size_t workspace_bytes, void* stream);
int geo4d_lad_fit(const float* q, const float* target, int G, long n, const unsigned char* active, float lr, int max_iters, float tol,
                  float* st_out, float* info_out, void* workspace, size_t workspace_bytes, void* stream);
int geo4d_lad_delta(const float* q, const float* target, const float* conf, const float* st, int G, long n, float conf_thr,
                    float conf_clamp, float q_thr, unsigned* counts, void* stream);

/* Video-depth evaluation against ground truth (dust3r/depth_eval.py depth_evaluation :147-355 as scripts/evaluation/infer_geo4d.py:514-545
 * calls it; geo4d_amd/evaluation.py). All arrays fp32 on the device, n elements of the flattened [T][H][W] sequence, n < 2^32.
 *   geo4d_bicubic_resize: y [T][OH][OW] = torch.nn.functional.interpolate(x [T][h][w], (OH, OW), "bicubic", align_corners=False) — what
 *     torchvision.transforms.Resize(BICUBIC) does to a float tensor under the reference's torch 2.0 / torchvision 0.15 (antialias off):
 *     a = -0.75, border-clamped taps, no output clamp.
 *   geo4d_masked_select: (pred_out, gt_out)[0, *count) = (clamp(pred, pre_min, pre_max), gt)[valid], valid = gt > 0 && gt < max_depth
 *     (max_depth = +INFINITY: no upper bound) && (mask == NULL || mask[i]), in index order (= torch boolean indexing); *count is a device
 *     int64. pred_out / gt_out hold n floats. workspace: geo4d_masked_select_workspace(n) bytes, 4-byte aligned.
 *   geo4d_depth_metrics: one pass over the full-size pred / gt with st = (s, t) read from the device. Metric pixels: gt > 0 && gt < max_depth
 *     && (custom_mask == NULL || custom_mask[i]); a = clamp(s * clamp(pred, pre_min, pre_max) + t, post_min, post_max); sums [8] fp64 =
 *     {sum |a-g|/g, sum (a-g)^2/g, sum (a-g)^2, sum (log a' - log g)^2, #(delta < 1.25), #(< 1.25^2), #(< 1.25^3), #pixels} with
 *     a' = max(a, 1e-5) and delta = max(a'/g, g/a') (:283-317). err_map [n] = |s pred + t - g| / g where gt > 0 && gt < max_depth, else 0;
 *     aligned [n] (may be NULL) = s pred + t (:320-335). Unused clips are -INFINITY / +INFINITY. workspace:
 *     geo4d_depth_metrics_workspace(n) bytes, 8-byte aligned. Deterministic (fixed-order reductions, no atomics). */
int geo4d_bicubic_resize(const float* x, float* y, int T, int h, int w, int OH, int OW, void* stream);
size_t geo4d_masked_select_workspace(long n);
int geo4d_masked_select(const float* pred, const float* gt, long n, float max_depth, const unsigned char* mask, float pre_min, float pre_max,
                        float* pred_out, float* gt_out, long* count, void* workspace, size_t workspace_bytes, void* stream);
size_t geo4d_depth_metrics_workspace(long n);
int geo4d_depth_metrics(const float* pred, const float* gt, long n, float max_depth, const unsigned char* custom_mask, const float* st,
                        float pre_min, float pre_max, float post_min, float post_max, double* sums, float* err_map, float* aligned,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Scene export (dust3r/demo.py get_3D_model_from_scene :56-86 on an aligned scene; geo4d_amd/scene_export.py). n images of H x W,
 * n * H * W < 2^31; every array on the device, image-major [n][H][W](...).
 *   geo4d_scene_clean: clean_pointcloud (dust3r/cloud_opt/base_opt_group.py:630-665) IN PLACE on conf [n][H][W] fp32. pts3d [n][H][W][3]
 *     world points, depth [n][H][W], mats [n][21] = rows 0..2 of the 4x4 world-to-camera matrix (12) then the 3x3 intrinsics (9),
 *     row-major. For i = 0 .. n-1 in order, for j != i ascending: pixel p of i goes to camera j, (u, v) = rint((K p)[:2] / (K p)[2]);
 *     where z > 0, 0 <= u < W, 0 <= v < H, z < (1 - tol) depth[j][v][u] and conf[i][p] < conf[j][v][u], conf[i][p] = min(conf[i][p],
 *     bad_conf). Rows j < i are read already cleaned, rows j > i as given (the reference's loop order). 0 <= tol < 1. n launches.
 *   geo4d_scene_points: (pts_out [*count][3], rgba_out [*count][4] u8) = (pts3d, rgb)[mask] in image-major raster order (mask NULL:
 *     every pixel); RGBA = clip(c * 255 + 0.5, 0, 255) truncated, alpha 255. rgb [n][H][W][3] fp32 and rgba_out are both set or both
 *     NULL; rgba_out 4-byte aligned. *count is a device int64; the outputs hold n H W rows. workspace: geo4d_scene_points_workspace bytes.
 *   geo4d_scene_mesh_faces: faces [*count][3] int32 = pts3d_to_trimesh + cat_meshes (dust3r/viz.py:40-90): per image i the blocks
 *     (tl, tr, bl), (bl, tr, tl), (tr, bl, br), (br, bl, tr) over the (H-1) x (W-1) quads in raster order, kept when all three vertices
 *     are valid in mask [n][H][W] (NULL: all), vertex ids + i H W. faces holds 4 n (H-1)(W-1) rows; H, W >= 2.
 *     workspace: geo4d_scene_mesh_faces_workspace bytes, 4-byte aligned. */
int geo4d_scene_clean(float* conf, const float* pts3d, const float* depth, const float* mats, int n, int H, int W, double tol, float bad_conf,
                      void* stream);
size_t geo4d_scene_points_workspace(int n, int H, int W);
int geo4d_scene_points(const float* pts3d, const float* rgb, const unsigned char* mask, int n, int H, int W, float* pts_out,
                       unsigned char* rgba_out, long* count, void* workspace, size_t workspace_bytes, void* stream);
size_t geo4d_scene_mesh_faces_workspace(int n, int H, int W);
int geo4d_scene_mesh_faces(const unsigned char* mask, int n, int H, int W, int* faces, long* count, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Frames of the aligned scene: z-buffered point splats (geo4d_amd/csrc/render.hip, geo4d_amd/render.py). Nothing of the reference is
 * replaced (it shows a scene in a browser); the rules are this project's own, restated in numpy in tests/render_restatement.py.
 *   V views of H x W pixels, V * H * W < 2^31. N points, 0 < N < 2^32 - 1, in whole images of pts_per_image points: image s holds the
 *   points s * pts_per_image .. ; a point's id is its row. Device arrays: points [N][3] fp32, mask [N] bytes (NULL: all), radius [N]
 *   fp32 world radii (NULL: one pixel per point), colors [N][3] fp32 in [0, 1], views [V][16] fp32 = rows 0..2 of the world-to-camera
 *   matrix (12, row-major) then fx, fy, cx, cy. HOST arrays: view_src_ptr [V + 1] and view_src, the CSR list of source images per view
 *   (rising from 0, every index < N / pts_per_image, checked before any launch), and background [3].
 *   workspace: geo4d_render_workspace bytes for n_entries = view_src_ptr[V], 8-byte aligned = two key buffers [V][H][W] uint64 (every
 *     call leaves its result in the first) and the device copy of the source lists.
 *   geo4d_render_splat: the key buffer := all ones, then for every view and every point of its source images (one launch, order
 *     irrelevant): xc = ((r00 X + r01 Y) + r02 Z) + t0, likewise yc, zc, no FMA; the point is dropped when masked out, when a world or
 *     camera coordinate is not finite, or when zc <= near; u = fx (xc / zc) + cx, v = fy (yc / zc) + cy (pixel i sits at coordinate i);
 *     side s = 1, or with radius min(max_size, max(1, ceil(2 radius fx / zc))), 1 <= max_size <= 64; columns x0 .. x0 + s - 1 with
 *     x0 = floor(u - 0.5 (s - 1) + 0.5), rows likewise, clipped to the image; every covered pixel takes the unsigned 64-bit minimum
 *     (a vector atomic) of key = float_bits(zc) << 32 | id: the nearest point, at equal depth the lower id, whatever the arrival order.
 *   geo4d_render_fill: `passes` times, every empty pixel (all ones) takes the minimum key of its 3 x 3 neighbours inside its view.
 *   geo4d_render_resolve: per pixel rgb [V][H][W][3] u8 = clip(c * 255 + 0.5, 0, 255) truncated of the winner's colour (the rule of
 *     geo4d_scene_points) or of background, depth [V][H][W] fp32 = zc or 0, index [V][H][W] int32 = id or -1 (hence N < 2^31 here);
 *     any of the three may be NULL, not all. */
size_t geo4d_render_workspace(int V, int H, int W, long n_entries);
int geo4d_render_splat(const float* points, const unsigned char* mask, const float* radius, long N, long pts_per_image, const float* views,
                       const int* view_src_ptr, const int* view_src, int V, int H, int W, float near, int max_size, void* workspace,
                       size_t workspace_bytes, void* stream);
int geo4d_render_fill(int V, int H, int W, int passes, void* workspace, size_t workspace_bytes, void* stream);
int geo4d_render_resolve(const float* colors, long N, const float* background, int V, int H, int W, unsigned char* rgb, float* depth,
                         int* index, const void* workspace, size_t workspace_bytes, void* stream);

/* Triangle meshes in the renderer: an exact raster into the splats' key buffer and a deferred-shading resolve
 * (geo4d_amd/csrc/render_mesh.hip, geo4d_amd/render.py render_mesh). The rule is this project's own, restated in numpy in
 * tests/render_mesh_restatement.py; coverage is integer arithmetic, every float operation is + - * / or a correctly rounded conversion
 * or square root in the written order, no FMA.
 *   Device arrays: vertices [Nv][3] fp32 world coordinates, faces [T][3] int32, face_mask [T] bytes (NULL: all), views [V][16] as above;
 *   every view draws the whole mesh. H, W <= 16384. Per (view, triangle t):
 *   1 drop it when masked out, when an index is outside [0, Nv) (checked on the device, nothing is read out of bounds), or unless every
 *     vertex has finite camera coordinates (the splat's xc, yc, zc) and zc > near: a triangle that crosses the near plane is dropped,
 *     there is no clipping;
 *   2 guard band: with u = fx (xc / zc) + cx, v likewise, drop it unless fabsf(u) < 65536 and fabsf(v) < 65536 at all three vertices,
 *     decided in float (NaN drops);
 *   3 snap: X = (long)floorf(u * 256.f + 0.5f), Y likewise (8 sub-pixel bits); pixel (x, y) is sampled at S = (256 x, 256 y);
 *   4 int64 edge functions edge(A, B, S) = (Bx - Ax)(Sy - Ay) - (By - Ay)(Sx - Ax): E0 = edge(P1, P2, S), E1 = edge(P2, P0, S),
 *     E2 = edge(P0, P1, S), A = edge(P0, P1, P2); every value stays below 2^51;
 *   5 A == 0 drops it; with cull_back, A > 0 drops it (a front face is counter-clockwise as seen: A < 0 with y down); if A < 0 negate A
 *     and every E_k;
 *   6 candidates x = max(0, (minX + 255) >> 8) .. min(W - 1, maxX >> 8), y likewise; covered iff E0 >= 0 && E1 >= 0 && E2 >= 0: every
 *     edge inclusive, no top-left rule, two triangles sharing an edge both claim its pixels and the depth test decides;
 *   7 iz_k = 1.f / zc_k, w_k = (float)((double)E_k / (double)A), q = ((w0 iz0) + (w1 iz1)) + (w2 iz2), zc = 1.f / q (perspective
 *     correct); the pixel is skipped unless zc > 0;
 *   8 one unsigned 64-bit atomic minimum of key = float_bits(zc) << 32 | (id_base + t) on the view's pixel, id_base + T < 2^32 - 1:
 *     with id_base = the point count a point beats a triangle at equal depth, and a lower face a higher one.
 *   geo4d_render_raster: `workspace` is the key buffer of geo4d_render_workspace; clear = 1 sets it to all ones first (a mesh alone),
 *     clear = 0 draws into what splat and fill left (fill runs BEFORE the raster: a copied triangle key would have no barycentrics). A
 *     (view, triangle) whose clipped bounding box holds more than large_area pixels is appended to `list` (geo4d_render_raster_workspace
 *     (capacity) bytes, 8-byte aligned: an 8-byte count, zeroed here, then capacity int pairs) and drawn by a second launch, one wave per
 *     entry; when the list is full the appending thread draws the triangle itself. The image depends on none of this.
 *   geo4d_render_resolve_mesh: a key with id < N is a point (as geo4d_render_resolve; colors may be NULL when N == 0); id >= N + T reads
 *     nothing and gives background; a triangle key, t = id - N, repeats steps 1 to 7 for its pixel (same integers, same w_k), depth is
 *     the key's, b_k = (w_k iz_k) zc, colour c = (b0 c0 + b1 c1) + b2 c2 per channel with c_k the vertex colour: vertex_rgba [Nv][4] u8
 *     as (float)u8 / 255.f (alpha ignored), or vertex_rgb [Nv][3] fp32 as given, or, with both NULL, the HOST array mesh_color [3].
 *     shade > 0 (at most 1): flat headlight shading with the camera-space edges e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2 (nx = e1y e2z -
 *     e1z e2y and cyclic), len2 = (nx nx + ny ny) + nz nz, lam = len2 > 0 ? fabsf(nz) / sqrtf(len2) : 0 (correctly rounded), g = (1 -
 *     shade) + shade lam, colour = c g. Outputs as geo4d_render_resolve (rgb quantised the same way) and face [V][H][W] int32 = t or
 *     -1; index is -1 where a triangle won. Any output may be NULL, not all. */
size_t geo4d_render_raster_workspace(long capacity);
int geo4d_render_raster(const float* vertices, long Nv, const int* faces, long T, const unsigned char* face_mask, const float* views,
                        int V, int H, int W, float near, int cull_back, long id_base, int clear, int large_area, void* workspace,
                        size_t workspace_bytes, void* list, size_t list_bytes, void* stream);
int geo4d_render_resolve_mesh(const float* colors, long N, const float* vertices, long Nv, const int* faces, long T,
                              const unsigned char* vertex_rgba, const float* vertex_rgb, const float* mesh_color, const float* views,
                              float near, float shade, const float* background, int V, int H, int W, unsigned char* rgb, float* depth,
                              int* index, int* face, const void* workspace, size_t workspace_bytes, void* stream);

/* Which pixels of the aligned scene moved: geometric votes between the images (geo4d_amd/csrc/motion.hip, geo4d_amd/motion.py). Nothing
 * of the reference is replaced (it fills dynamic_mask_{i}.png from optical flow and SAM2); the rule is this project's own, restated in
 * numpy in tests/motion_restatement.py.
 *   n images of H x W pixels, n * H * W < 2^31. Device arrays: depth [n][H][W] fp32, valid [n][H][W] bytes (NULL: all), pts3d
 *   [n][H][W][3] fp32 world points, views [n][16] fp32 = rows 0..2 of each image's world-to-camera matrix (12, row-major) then fx, fy,
 *   cx, cy, votes [n][H][W][3] u8. workspace: geo4d_motion_workspace bytes, 8-byte aligned = one (dmin, dmax) fp32 pair per pixel.
 *   geo4d_motion_range: for every image j and pixel q, dmin / dmax = the minimum / maximum of depth[j] over the valid pixels of q's
 *     3 x 3 neighbourhood inside the image (a NaN depth never wins; nothing to compare leaves (+inf, -inf)); an invalid q gets
 *     dmin = NaN, which is how geo4d_motion_votes sees the mask.
 *   geo4d_motion_votes: for every image i, every valid pixel p with a finite world point (X, Y, Z) and every j with
 *     0 < |j - i| <= radius, 0 <= j < n (1 <= radius <= 127): xc = ((r00 X + r01 Y) + r02 Z) + t0, likewise yc, zc, no FMA; skipped
 *     unless all three are finite and zc > near (near >= 0); u = fx (xc / zc) + cx, v = fy (yc / zc) + cy; column = floor(u + 0.5),
 *     row = floor(v + 0.5) (pixel k sits at coordinate k), inside / outside decided in float before any cast; skipped when outside or
 *     when j's pixel there is invalid. With lo = 1 - tol, hi = 1 + tol in fp32 (0 < tol < 1): free if zc < dmin lo (camera j sees past
 *     the place where the point was), else occluded if zc > dmax hi (something is in front: no evidence), else consistent.
 *     votes[i][p] = (consistent, free, occluded) counts, each <= 2 radius; (0, 0, 0) for invalid pixels. One writer per byte, no atomics.
 *   Bad sizes, radius, tol, near and null pointers return -EINVAL before any launch. */
size_t geo4d_motion_workspace(int n, int H, int W);
int geo4d_motion_range(const float* depth, const unsigned char* valid, int n, int H, int W, void* workspace, size_t workspace_bytes,
                       void* stream);
int geo4d_motion_votes(const float* pts3d, const float* views, int n, int H, int W, int radius, float tol, float near,
                       unsigned char* votes, const void* workspace, size_t workspace_bytes, void* stream);

/* The aligned scene's points merged into one cloud, one point per occupied voxel (geo4d_amd/csrc/fuse.hip, geo4d_amd/fusion.py). The
 * reference has no such step; the rule is this project's own, restated in numpy in tests/fusion_restatement.py.
 *   Device arrays: points [N][3] fp32, rgba [N][4] u8 (NULL: no colours), weight [N] fp32 (NULL: every weight is 1), mask [N] bytes
 *   (NULL: all); 0 <= N < 2^31; voxel v > 0 finite, fp32. All float arithmetic is fp32 in the written order, no FMA; only the final
 *   position is fp64.
 *   Which points take part: point i takes part iff mask[i], X, Y, Z are finite, its weight w (when given) is finite and > 0, and per
 *     axis the cell c = floorf(X / v) satisfies fabsf(c) < 2^20. A point that fails only the last condition is counted in *dropped;
 *     the others are skipped silently.
 *   Voxel key: (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), below 2^63; all ones marks an empty slot. Unsigned key order is
 *     lexicographic (cx, cy, cz) order.
 *   Per point: offset q_a = (int)clamp(floorf((X_a - c_a v) / v * 65536.f + 0.5f), 0.f, 65535.f) (clamped as a float, then cast),
 *     weight wq = (int)clamp(floorf(w * 128.f + 0.5f), 1.f, 32767.f).
 *   Per voxel, integer sums: count, sw = sum wq, sq_a = sum wq q_a, sc_k = sum wq rgba_k (k = 0..2), u64 each; N < 2^31, wq < 2^15,
 *     q < 2^16: no sum can overflow, and integer addition does not depend on the order the points arrive in.
 *   reduce 0 (mean): pos_a = (float)(((double)c_a + (double)sq_a / ((double)sw * 65536.0)) * (double)v); colour (sc_k + sw / 2) / sw
 *     in integers, alpha 255; weight (float)((double)sw / (128.0 * count)).
 *   reduce 1 (best): the input point of highest weight, the lowest row on ties (the unsigned 64-bit maximum of float_bits(w) << 32 |
 *     (0xffffffff - i)); position, colour and weight are copied bit for bit; count is still the voxel's count.
 *   workspace: geo4d_fuse_workspace bytes (0 for a capacity that is no power of two in 1 .. 2^32 or an unknown reduce), 8-byte
 *     aligned = an open-addressing table of `capacity` 64-bit keys (linear probing from a 64-bit mix of the key) and per slot 8 words
 *     (mean) or 2 (best) of accumulators. capacity >= N, so an insert always finds a slot.
 *   geo4d_fuse_insert: table := empty, *dropped := 0, then one launch over the points (64-bit vector atomics on global memory: CAS to
 *     claim a slot, add / max into it; no lane waits for another).
 *   geo4d_fuse_compact: *count := the number of occupied slots; their (key, slot) pairs go to keys_out / slots_out [max_pairs] in
 *     arrival order (pairs beyond max_pairs are counted, not written). The caller sorts them by key.
 *   geo4d_fuse_finalize: row m of the outputs = the voxel in slot order[m], 0 <= m < M <= N: points_out [M][3] fp32, rgba_out [M][4]
 *     u8 (NULL without colours), weight_out [M] fp32, count_out [M] int32. points / rgba / weight are the insert's (read by best).
 *   Null pointers, N < 0 or >= 2^31, a voxel that is not finite or <= 0, a capacity that is no power of two or < N, an unknown reduce
 *   and a workspace that is too small return -EINVAL before any device work. */
size_t geo4d_fuse_workspace(long capacity, int reduce);
int geo4d_fuse_insert(const float* points, const unsigned char* rgba, const float* weight, const unsigned char* mask, long N, float voxel,
                      int reduce, long capacity, long* dropped, void* workspace, size_t workspace_bytes, void* stream);
int geo4d_fuse_compact(long capacity, int reduce, long* keys_out, long* slots_out, long max_pairs, long* count, const void* workspace,
                       size_t workspace_bytes, void* stream);
int geo4d_fuse_finalize(const long* order, long M, const float* points, const unsigned char* rgba, const float* weight, long N, float voxel,
                        int reduce, long capacity, float* points_out, unsigned char* rgba_out, float* weight_out, int* count_out,
                        const void* workspace, size_t workspace_bytes, void* stream);

/* The static scene denoised: a truncated signed distance function (TSDF) over the voxels near a surface, averaged over every image that
 * sees them, and the surface points where it crosses zero (geo4d_amd/csrc/tsdf.hip, geo4d_amd/tsdf.py). The reference has no such step;
 * the rule is this project's own, restated in numpy in tests/tsdf_restatement.py.
 *   Device arrays: pts3d [n][H][W][3] fp32, depth [n][H][W] fp32, valid [n][H][W] bytes (NULL: all), views [n][16] fp32 exactly as
 *   geo4d_motion_votes takes them, centres [n][3] fp32 (the camera centres), rgba [n][H][W][4] u8 (NULL: no colours), weight [n][H][W]
 *   fp32 (NULL: every weight is 1); n, H, W > 0, n H W < 2^31; voxel v > 0 finite; truncation T = 1 .. 8 voxels, trunc = (float)T * v;
 *   near >= 0; min_weight > 0. All float arithmetic is fp32 in the written order, no FMA; only division, no sqrt.
 *   geo4d_tsdf_mark: table := empty, counters[0] (dropped) := counters[1] (overflow) := 0, then one launch over the pixels. Pixel (i, p)
 *     takes part iff it is valid, its point P and depth are finite and depth > near. d = P - C_i, s = (v * 0.5f) / depth; for
 *     k = -2T .. 2T the sample is P_a + ((float)k * s) * d_a (a step of v / 2 in camera z) and its cell floorf(sample_a / v). Keys are
 *     geo4d_fuse_insert's: (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), |c| < 2^20, all ones = empty, unsigned order = (cx, cy,
 *     cz) order; a sample whose cell is out of range is counted in dropped. workspace: geo4d_tsdf_workspace bytes (0 for a capacity
 *     that is no power of two in 1 .. 2^32), 8-byte aligned = `capacity` 64-bit keys, open addressing with linear probing from a 64-bit
 *     mix of the key: a relaxed read, a 64-bit CAS only on an empty slot, forward probing, no lane waits for another. A sample that
 *     has probed `capacity` slots without a home is counted in overflow and gives up (as does every lane that then sees overflow != 0):
 *     the caller must refuse the table. The marked set is a set: its content depends neither on arrival order nor on capacity.
 *   geo4d_tsdf_compact: *count := the number of occupied slots; their keys go to keys_out [max_keys] in arrival order (keys beyond
 *     max_keys are counted, not written). The caller sorts them: K[0..M).
 *   geo4d_tsdf_integrate: one thread per voxel m with centre X_a = ((float)c_a + 0.5f) * v; for j = 0 .. n-1 in that order:
 *     xc = ((r00 X + r01 Y) + r02 Z) + t0, likewise yc, zc; skipped unless all three are finite and zc > near; u = fx (xc / zc) + cx,
 *     v = fy (yc / zc) + cy; column = floorf(u + 0.5f), row = floorf(v + 0.5f), inside / outside decided in float before any cast;
 *     skipped unless j's pixel there is valid, its depth finite and its weight w finite and > 0; sd = depth - zc; skipped if
 *     sd < -trunc; t = fminf(1.f, sd / trunc); D += w * t; Wt += w; if also sd <= trunc: C_k += w * (float)rgba_k (k = 0..2), Wc += w.
 *     f_out[m] = D / Wt, weight_out[m] = Wt, rgba_out[m] = (u8)clamp(floorf(C_k / Wc + 0.5f), 0, 255) (0 when Wc == 0), alpha 255.
 *   geo4d_tsdf_count / geo4d_tsdf_write: voxel m is live iff Wt >= min_weight and |f| < 1. For live m and axis a = 0, 1, 2: m' = the
 *     row of key K[m] + (1 << 42, 1 << 21, 1)[a], by binary search; if it exists, is live and (f >= 0) != (f' >= 0), one point:
 *     X_a + (f / (f - f')) * v on axis a and the centre's coordinates on the other two, the colour of the voxel of smaller |f| (m on
 *     ties), weight fminf(Wt, Wt'). count writes counts[m] = 0 .. 3; write puts voxel m's points at rows first_row[m] .. of points_out
 *     [P][3], rgba_out [P][4] (NULL without colours) and weight_out [P], first_row = the exclusive prefix sum of counts and P their sum:
 *     rows in (m, a) order.
 *   Null pointers, bad sizes, a voxel that is not finite or <= 0, T outside 1 .. 8, near < 0, min_weight <= 0, a capacity that is no
 *   power of two and a workspace that is too small return -EINVAL before any device work. */
size_t geo4d_tsdf_workspace(long capacity);
int geo4d_tsdf_mark(const float* pts3d, const float* depth, const unsigned char* valid, const float* centres, int n, int H, int W, float voxel,
                    int trunc, float near, long capacity, long* counters, void* workspace, size_t workspace_bytes, void* stream);
int geo4d_tsdf_compact(long capacity, long* keys_out, long max_keys, long* count, const void* workspace, size_t workspace_bytes, void* stream);
int geo4d_tsdf_integrate(const long* keys, long M, const float* depth, const unsigned char* valid, const float* weight,
                         const unsigned char* rgba, const float* views, int n, int H, int W, float voxel, int trunc, float near, float* f_out,
                         float* weight_out, unsigned char* rgba_out, void* stream);
int geo4d_tsdf_count(const long* keys, long M, const float* f, const float* weight, float min_weight, int* counts, void* stream);
int geo4d_tsdf_write(const long* keys, long M, const float* f, const float* weight, const unsigned char* rgba, const long* first_row, long P,
                     float voxel, float min_weight, float* points_out, unsigned char* rgba_out, float* weight_out, void* stream);

/* The TSDF's surface as one indexed triangle mesh: naive surface nets, the dual method (geo4d_amd/csrc/tsdf_mesh.hip, geo4d_amd/tsdf.py
 * tsdf_mesh). The reference has no such step; the rule is this project's own, restated in numpy in tests/tsdf_mesh_restatement.py.
 *   Inputs: exactly what geo4d_tsdf_integrate leaves: keys K int64 [M] sorted (cell index + 2^20 in three 21-bit fields), f fp32 [M],
 *   weight Wt fp32 [M], rgba u8 [M][4] (NULL: no colours), plus the voxel v and min_weight. All arithmetic is fp32 in the written order,
 *   no FMA; only + - * / are used.
 *   Live is geo4d_tsdf_count's (Wt >= min_weight and |f| < 1); s(m) = f[m] >= 0; the step along axis a is E_a = (1 << 42, 1 << 21, 1)[a].
 *     A key field holds 1 .. 2^21 - 1 for a real cell: + E_a out of a full field carries into a field of value 0 and - E_a from 1 gives
 *     0, and no cell has either key, so no edge-of-grid test is needed in either direction.
 *   Cell m is the cube whose eight corners are the voxel centres with keys K[m] + ox E_0 + oy E_1 + oz E_2, o in {0, 1}^3, corner index
 *     4 ox + 2 oy + oz. It is complete iff all eight keys are in K and all eight voxels are live.
 *   Face: for voxel m and axis a let m' = the row of K[m] + E_a; the pair qualifies if m and m' are live and s(m) != s(m'). With
 *     b = (a + 1) % 3 and c = (a + 2) % 3 the four cells sharing that grid edge are r0 = m, r1 = m - E_b, r2 = m - E_b - E_c,
 *     r3 = m - E_c; one quad is emitted iff all four exist in K and are complete. If f[m] < 0 the ring is (r0, r1, r2, r3) (positive f
 *     is the free space in front of the surface, which is then on the + a side, and this ring is counter-clockwise seen from + a),
 *     otherwise (r0, r3, r2, r1); the two triangles are (q0, q1, q2) and (q0, q2, q3) of the ring, so front faces look toward the
 *     cameras. Quads are ordered by (m, a); triangle rows are 2 quad and 2 quad + 1.
 *   Vertex: a cell is used iff an emitted quad names it; used cells get the ids 0 .. V - 1 in order of m. A complete cell with a sign
 *     change but no emitted quad gets no vertex. For a = 0, 1, 2 and, within a, the four edges with the other two axes' offsets (0, 0),
 *     (1, 0), (0, 1), (1, 1) (lower axis first): p = the corner with o_a = 0, q = the corner with o_a = 1; if s(p) != s(q):
 *     t = f_p / (f_p - f_q), o with o_a replaced by t is added to S componentwise (S starts at 0, in this order), cnt += 1. The vertex is
 *     X0_k + (S_k / (float)cnt) * v with X0 = ((float)cell + 0.5f) * v. Colour: that of the corner with the smallest |f|, the lowest
 *     corner index on ties. Weight: the minimum Wt of the eight corners, by fminf in corner order.
 *   geo4d_tsdf_mesh_cells: complete[m] = 0 for a cell that is not complete, else 1 | 2 x0 | 4 x1 | 8 x2 with x_a = s(m) != s(m + E_a)
 *     (m + E_a is a corner of cell m). geo4d_tsdf_mesh_count: used := 0, then counts[m] = the quads of voxel m (0 .. 3) and used[r] = 1
 *     for the four ring cells of each. The caller forms first_quad and first_vertex = the exclusive prefix sums of counts
 *     and used, and Q, V = their sums. geo4d_tsdf_mesh_vertices writes vertex first_vertex[m] of every used cell to vertices_out [V][3],
 *     rgba_out [V][4] (NULL without colours) and weight_out [V]; geo4d_tsdf_mesh_faces writes the triangles of quad first_quad[m] .. to
 *     faces_out [2 Q][3] int32. One writer per row, no atomics: the output is a function of the inputs alone. A row offset outside the
 *     output writes nothing.
 *   Limits: M < 2^31, T = 2 Q. A grid face with four sign changes gives a mesh edge shared by four triangles: a property of the method.
 *   Null pointers, M < 0 or >= 2^31, Q > 3 M, V > M, a voxel that is not finite or <= 0 and min_weight <= 0 return -EINVAL before any
 *   device work. */
int geo4d_tsdf_mesh_cells(const long* keys, long M, const float* f, const float* weight, float min_weight, unsigned char* complete,
                          void* stream);
int geo4d_tsdf_mesh_count(const long* keys, long M, const unsigned char* complete, int* counts, unsigned char* used, void* stream);
int geo4d_tsdf_mesh_vertices(const long* keys, long M, const float* f, const float* weight, const unsigned char* rgba,
                             const unsigned char* used, const long* first_vertex, long V, float voxel, float* vertices_out,
                             unsigned char* rgba_out, float* weight_out, void* stream);
int geo4d_tsdf_mesh_faces(const long* keys, long M, const float* f, const unsigned char* complete, const int* counts, const long* first_quad,
                          const long* first_vertex, long Q, long V, int* faces_out, void* stream);

/* The connected pieces of an indexed triangle mesh, and the mesh of a chosen set of its faces (geo4d_amd/csrc/mesh_components.hip,
 * geo4d_amd/mesh.py): what removes the detached debris a TSDF of noisy depth leaves. The reference has no such step; the rule is this
 * project's own, restated in numpy in tests/mesh_components_restatement.py. Integer arithmetic throughout: every output is a function of
 * the inputs alone; permuting the faces permutes face_component and leaves the other outputs equal.
 *   Inputs: faces int32 [T][3], the vertex count Nv, face_mask u8 [T] (NULL: every face).
 *   Valid: face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv), which is decided before
 *     anything is read or written through them. A valid face may repeat an index: (a, a, b) connects a and b, (a, a, a) touches a alone.
 *   Connected: two vertices are connected iff a chain of valid faces links them, consecutive faces sharing at least one vertex (vertex
 *     connectivity, not edge connectivity).
 *   Labels: a vertex that no valid face names is untouched: vertex_component = -1. Every other vertex belongs to exactly one component;
 *     the root of a component is its smallest vertex index; components are numbered 0 .. C - 1 in ascending order of root.
 *     face_component[t] is the component of the face's vertices, -1 for a face that is not valid. component_vertices int32 [C] and
 *     component_faces int32 [C] count the touched vertices and the valid faces. A component's size is its face count.
 *   Selection: given keep_face u8 [T], face t is kept iff keep_face[t] != 0 and its indices lie in [0, Nv); a vertex is kept iff a kept
 *     face names it. Kept vertices and kept faces keep their relative order; faces are rewritten to the new vertex rows; vertex_index
 *     int32 [V'] is the old row of every new one.
 *   geo4d_mesh_components_hook: touched u8 [Nv] := 0, parent int32 [Nv] := identity, then one thread per face joins (i0, i1) and (i1, i2)
 *     in a lock-free union-find (geo4d_amd/csrc/union_find.h: parent[x] <= x always, the larger root is linked under the smaller by a
 *     compare-and-swap on a root, paths are halved by atomic minimum; every loop turn finishes or moves to a strictly smaller index and
 *     no thread waits for another) and stores touched = 1 for its vertices. geo4d_mesh_components_flatten, after it: root_out [Nv] = the
 *     smallest index of v's component, -1 for an untouched v; is_root_out u8 [Nv] = (root_out[v] == v). The caller forms first_component
 *     = the exclusive prefix sum of is_root_out (int64) and C = its sum. geo4d_mesh_components_count: component_* := 0, then
 *     vertex_component [Nv], face_component [T] (one writer per row) and the two counts (integer atomic adds).
 *     geo4d_mesh_select_mark: keep_vertex u8 [Nv] := 0, then 1 for the vertices of kept faces; kept_face u8 [T] = face t is kept. The
 *     caller forms first_vertex, first_face = the exclusive prefix sums of the two (int64) and V', T' = their sums.
 *     geo4d_mesh_select_gather writes vertices_out fp32 [V'][3], rgba_out u8 [V'][4] and weight_out fp32 [V'] (each NULL: not wanted),
 *     faces_out int32 [T'][3] and vertex_index int32 [V']; one writer per row; a row offset outside the output writes nothing.
 *   T == 0 or Nv == 0 (and C == 0, V' == 0 or T' == 0) launch nothing: every label is then -1 and every output empty, which is the
 *     caller's to write. Limits: T < 2^31, Nv < 2^31; vertex connectivity only; no areas, no bounding boxes.
 *   Null pointers (rgba, weight, their outputs and face_mask excepted), T or Nv < 0 or >= 2^31, C > Nv, V' > Nv and T' > T return
 *   -EINVAL before any device work. */
int geo4d_mesh_components_hook(const int* faces, long T, long Nv, const unsigned char* face_mask, int* parent, unsigned char* touched,
                               void* stream);
int geo4d_mesh_components_flatten(const int* parent, const unsigned char* touched, long Nv, int* root_out, unsigned char* is_root_out,
                                  void* stream);
int geo4d_mesh_components_count(const int* faces, long T, long Nv, const unsigned char* face_mask, const int* root,
                                const long* first_component, long C, int* vertex_component, int* face_component, int* component_vertices,
                                int* component_faces, void* stream);
int geo4d_mesh_select_mark(const int* faces, long T, long Nv, const unsigned char* keep_face, unsigned char* keep_vertex,
                           unsigned char* kept_face, void* stream);
int geo4d_mesh_select_gather(const float* vertices, const unsigned char* rgba, const float* weight, const int* faces, long T, long Nv,
                             const unsigned char* keep_vertex, const unsigned char* kept_face, const long* first_vertex,
                             const long* first_face, long V, long F, float* vertices_out, unsigned char* rgba_out, float* weight_out,
                             int* faces_out, int* vertex_index, void* stream);

/* The corner table of an indexed triangle mesh - for each vertex, the corners of the faces around it - and its three consumers:
 * boundary vertices, the Taubin (lambda | mu) smoothing step and area-weighted vertex normals (geo4d_amd/csrc/mesh_smooth.hip,
 * geo4d_amd/mesh.py). The reference has no such step; the rule is this project's own, restated in numpy in
 * tests/mesh_smooth_restatement.py. The table is sorted and therefore a function of the mesh alone; the float outputs are gathered per
 * vertex by one thread in the table's order (no float atomics), so they are bitwise reproducible.
 *   Inputs: vertices fp32 [Nv][3], faces int32 [T][3], face_mask u8 [T] (NULL: every face).
 *   Valid: face t is valid iff face_mask[t] != 0 (or there is no mask) and its three indices lie in [0, Nv), which is decided before
 *     anything is read or written through them. A valid face may repeat an index.
 *   Arithmetic: fp32 in the written order, contraction into FMAs off, only + - * / and sqrtf, each correctly rounded.
 *   1. Corner table: an entry is e = 3 t + k for a valid face t and corner k; it belongs to vertex faces[t][k]. offsets int32 [Nv + 1]
 *     is the exclusive prefix sum of the entries per vertex; corners int32 [E] holds each vertex's entries ascending in e. A face that
 *     names v twice appears twice in v's row. 3 T >= 2^31 is refused.
 *   2. Neighbour list of v: walk v's row in order; for each entry (t, k) take a = faces[t][(k + 1) % 3], then b = faces[t][(k + 2) % 3];
 *     skip those equal to v. m is the list's length.
 *   3. Boundary: boundary[v] = 1 iff some id occurs exactly once in v's neighbour list, else 0; an empty list gives 0. A neighbour
 *     across an edge that three or four triangles share occurs three or four times and does not make v a boundary vertex.
 *   4. Step with factor s: S = 0; for each w of the list in order S_c = S_c + p[w]_c; then p'[v]_c = p[v]_c + s * (S_c / (float) m -
 *     p[v]_c). v keeps its position bit for bit if m = 0 or pinned[v] != 0. A step reads one buffer and writes another (Jacobi).
 *   5. Smoothing (the caller's loop): each iteration runs a step with lam and, if mu != 0, a step with mu. The weights count faces: a
 *     neighbour seen from two faces counts twice (the mean of the opposite edges' midpoints). Non-finite coordinates propagate as IEEE
 *     arithmetic says.
 *   6. Normals: n(t) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) with e1 = p1 - p0, e2 = p2 - p0 in the face's own
 *     vertex order (its length is twice the area: the weighting is by area). N = 0; for each entry of v's row in order N_c = N_c +
 *     n(t)_c; len2 = (Nx Nx + Ny Ny) + Nz Nz; the result is N_c / sqrtf(len2) if len2 > 0 and finite in float, else (0, 0, 0), which
 *     a vertex with an empty row gets.
 *   7. Invariance: offsets, boundary and the multiset of each row are integer functions of the mesh, invariant under a permutation
 *     of the faces up to the renaming of t. The float outputs are functions of the mesh as given: permuting the faces reorders the
 *     sums and may change last bits.
 *   geo4d_mesh_adjacency_count: degree int32 [Nv], zeroed by the caller, += 1 per corner of a valid face (integer atomics). The caller
 *     forms offsets [Nv + 1] = 0 followed by the inclusive prefix sum of degree, and E = offsets[Nv]. geo4d_mesh_adjacency_fill: cursor
 *     int32 [Nv], zeroed by the caller; corners [E] receives every entry in its vertex's row, in arbitrary order within the row.
 *     geo4d_mesh_adjacency_sort: corners_out [E] (another buffer) = every row of corners_in ascending; a row of at most long_row
 *     entries is sorted by one thread, a longer one by one wave (both give the same table). geo4d_mesh_boundary: boundary u8 [Nv],
 *     one writer per vertex, the same split by long_row. geo4d_mesh_smooth_step: vertices_out fp32 [Nv][3] (another buffer), pinned
 *     u8 [Nv] or NULL. geo4d_mesh_vertex_normals: normals_out fp32 [Nv][3]. One thread per vertex walks its row in the last two: time is
 *     linear in the largest valence. Rows outside [0, E], entries outside [0, 3 T) and indices outside [0, Nv) are skipped.
 *   T == 0 or Nv == 0 (and E == 0 for fill and sort) launch nothing; the outputs are then the caller's to write.
 *   Null pointers (face_mask and pinned excepted, and the consumers' corners when E == 0: an empty table has no storage), T or Nv
 *   < 0 or >= 2^31, 3 T >= 2^31, E < 0 or > 3 T, long_row < 0, an output that is its own input, and s not finite return -EINVAL
 *   before any device work. */
int geo4d_mesh_adjacency_count(const int* faces, long T, long Nv, const unsigned char* face_mask, int* degree, void* stream);
int geo4d_mesh_adjacency_fill(const int* faces, long T, long Nv, const unsigned char* face_mask, const int* offsets, long E, int* cursor,
                              int* corners, void* stream);
int geo4d_mesh_adjacency_sort(const int* offsets, long T, long Nv, long E, const int* corners_in, int* corners_out, int long_row,
                              void* stream);
int geo4d_mesh_boundary(const int* faces, long T, long Nv, const int* offsets, const int* corners, long E, int long_row,
                        unsigned char* boundary, void* stream);
int geo4d_mesh_smooth_step(const float* vertices, const int* faces, long T, long Nv, const int* offsets, const int* corners, long E,
                           const unsigned char* pinned, float s, float* vertices_out, void* stream);
int geo4d_mesh_vertex_normals(const float* vertices, const int* faces, long T, long Nv, const int* offsets, const int* corners, long E,
                              float* normals_out, void* stream);

/* For every query point, the nearest reference point within a radius and the number of reference points within it, on a grid of cells
 * of side radius (geo4d_amd/csrc/nearest.hip, geo4d_amd/nearest.py): what the cloud metrics of geo4d_amd/evaluation.py and the radius
 * outlier removal of geo4d_amd/fusion.py stand on. The reference has no such step; the rule is this project's own, restated in numpy in
 * tests/nearest_restatement.py. Arithmetic: fp32 in the written order, contraction into FMAs off, only + - * / and floorf, each
 * correctly rounded, so no comparison with the restatement has a tolerance.
 *   Inputs: reference fp32 [Nr][3] with reference_mask u8 [Nr] (NULL: every row), query fp32 [Nq][3] with query_mask likewise, the
 *     radius r > 0 with r2 = r * r finite in fp32, exclude_same_row (0 / 1); Nr, Nq < 2^31.
 *   1. Cells: the cell side is r; a point's cell is c_a = floorf(X_a / r); the cell takes part iff fabsf(c_a) < 2^20 on every axis and
 *     its key is (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), as for the fusion: unsigned key order is (cx, cy, cz) order.
 *   2. Who takes part: a point (reference or query) takes part iff its mask is set, its coordinates are finite and its cell takes part.
 *     A point that fails only the last condition is counted in `dropped`; the others are skipped silently. A query that takes no part
 *     gets index = -1, dist2 = +inf, count = 0.
 *   3. Candidates of query i: the taking-part reference rows j whose integer cell differs from the query's by at most 1 on every axis,
 *     without j = i when exclude_same_row. Cells outside the grid (|c| >= 2^20) do not exist and are skipped; they are never reached
 *     through a carry between the fields of a key.
 *   4. Distance: dx = Qx - Rx, likewise dy, dz; d2 = (dx dx + dy dy) + dz dz; j is within iff d2 <= r2.
 *   5. Per query: count int32 = the number of candidates within; index int32 = the within candidate with the smallest (d2, j) in
 *     lexicographic order (the lowest original row wins on ties), or -1; dist2 fp32 = its d2, or +inf.
 *   6. Every output is a minimum or an integer count over a set, so it depends neither on the order the candidates are visited in nor
 *     on the run: two runs are equal bit for bit. Permuting the reference rows leaves dist2 and count unchanged.
 *   7. Against "every taking-part reference with d2 <= r2" the restriction to neighbouring cells changes nothing in exact arithmetic;
 *     floorf(X / r) rounds, so a query can differ only where a reference lies within rounding of r from it (measured: none of 3 000
 *     queries, six inputs, tests/test_nearest_cpu.py).
 *   geo4d_nn_keys: keys_out int64 [N] = the key of a taking-part point, all ones for any other (after every real key in unsigned
 *     order; first in a signed sort); dropped int64 [1] := the count of rule 2 (zeroed by the call; one integer atomic add per
 *     workgroup). The caller sorts the keys stably and forms the grid of the reference: cell_keys int64 [M] sorted and unique,
 *     cell_start int32 [M + 1] = the exclusive prefix sum of the points per cell, Nt = cell_start[M] the taking-part points.
 *     geo4d_nn_gather: for k < Nt, sorted_out fp32 [Nt][3] = points[order[k]] and row_out int32 [Nt] = order[k], where order int64
 *     [Nt] lists the taking-part rows in (key, row) order; an entry outside [0, N) gives row -1 and NaN coordinates.
 *     geo4d_nn_query: query_order int64 [Nq] lists the query rows, the Nq_taking taking-part ones first and sorted by their own key
 *     (so that a wave's lanes share cells); one thread per entry writes the three outputs of its row: the rule above for the first
 *     Nq_taking, (-1, +inf, 0) for the others. Nine lower-bound searches of cell_keys per query (the three cells of a column are
 *     consecutive in key order), each followed by a walk over the column's contiguous range of ref_sorted. Every loop is counted: 3 x 3
 *     columns, at most 32 halvings, at most 3 cells, at most Nt points; no thread waits for another. A cell_start outside [0, Nt] and
 *     a ref_row outside [0, Nr) are skipped and never dereferenced; a query_order entry outside [0, Nq) writes nothing.
 *   N = 0, Nt = 0 and Nq = 0 launch nothing. Limits: one nearest neighbour, int32 indices; time grows with the points per cell.
 *   Null pointers (the masks excepted, and what an extent of 0 leaves without storage), sizes < 0 or >= 2^31, Nt > N, Nq_taking > Nq,
 *   M > Nt, Nt > Nr, a radius that is not finite and > 0 or whose square is not finite in fp32, exclude_same_row other than 0 / 1 and
 *   an output that is an input or another output return -EINVAL before any device work. */
int geo4d_nn_keys(const float* points, const unsigned char* mask, long N, float radius, long* keys_out, long* dropped, void* stream);
int geo4d_nn_gather(const float* points, const long* order, long Nt, long N, float* sorted_out, int* row_out, void* stream);
int geo4d_nn_query(const float* query, const long* query_order, long Nq_taking, long Nq, const long* cell_keys, const int* cell_start,
                   long M, const float* ref_sorted, const int* ref_row, long Nt, long Nr, float radius, int exclude_same_row,
                   int* index_out, float* dist2_out, int* count_out, void* stream);

/* z-shift and focal of point maps from the maps alone (geo4d_amd/csrc/focal_shift.hip). replaces utils.geometry.point_map_to_depth ->
 * solve_optimal_shift_focal(..., ransac_iters=None) (utils/geometry.py:162-270: nearest down-sampling, then scipy least_squares from
 * shift 0 per map on the host), as init_im_poses.align_group_prefix (:244-271) calls it. Per map b, over the selected pixels:
 *   minimise E(shift) = sum | f xy / (z + shift) - uv |^2 with f = sum(p.uv) / sum(p.p), p = xy / (z + shift), uv = image_plane_uv(W, H)
 *   (utils/geometry.py:217-229, computed in the kernel); local minimum reached downhill from shift 0 with z + shift > 0 kept for every
 *   selected pixel (when shift 0 already violates that, the start is min z + shift = 1).
 * points: fp32, map b at points + b * map_stride, each map a dense [H][W][3]; weight (may be NULL: every pixel) fp32, map b at
 * weight + b * weight_stride, dense [H][W]: a pixel is selected when weight > thr; z_offset (may be NULL) one device fp32 added to every
 * z; the (h_lr, w_lr) grid samples the maps at F.interpolate(mode="nearest")'s source indices, (H, W) = every pixel. iters: solver
 * iterations, all enqueued at once (two launches each; a converged map skips its pixel passes); nothing is read back in between.
 * Outputs (device): shift [B], focal [B] fp32 (the normalised optim_focal: fov_x = 2 atan(W / diagonal / focal)), status [B] int32 = 0 ok,
 * 1 fewer than 3 selected pixels (shift 0, focal 1), 2 non-finite / non-positive result; outputs are finite in every case.
 * workspace: geo4d_focal_shift_workspace bytes, 8-byte aligned, holds ALL solver state. Deterministic (fixed-order fp64 reductions). */
size_t geo4d_focal_shift_workspace(int B, int h_lr, int w_lr);
int geo4d_focal_shift(const float* points, long map_stride, const float* weight, long weight_stride, float thr, const float* z_offset, int B,
                      int H, int W, int h_lr, int w_lr, int iters, float* shift, float* focal, int* status, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Batched RANSAC-PnP, B images x C candidate focals (geo4d_amd/csrc/pnp.hip): geo4d_amd/pnp.py's fast_pnp / solve_pnp_ransac hypothesis
 * for hypothesis, with the sampler's tables (pnp.sample_tables) drawn on the host. Everything but the scalars is on the device.
 *   points fp32, image b at points + b * image_stride, dense [H*W][3] world points; conf fp32, image b at conf + b * conf_stride, dense
 *   [H*W]: a pixel is masked in when conf > thr. Pixel coordinates are the raster grid (x = column, y = row). cand_focals fp64 [B][C],
 *   1 <= C <= 64, B * C <= 65535; (ppx, ppy) the principal point; reproj the inlier threshold in pixels; iterations the RANSAC cap; sample must be 6.
 *   n [B] int32: masked pixels of image b as the caller counted them (the tables depend on it; a different count fails the image);
 *   m [B] int32: length of image b's sub-sample, 6 <= m <= min(n, max_points); sub [B][max_points] int32: sorted ranks into the masked
 *   pixels in raster order; draws [B][iterations][6] int32 into sub. Indices are range-checked on the device.
 * Outputs: focal [B] and c2w [B][4][4] fp64 (winning candidate: strictly most inliers over all n masked pixels, ties to the first;
 *   camera-to-world) are WRITTEN ONLY for an image with status 0, so the caller's values survive a failure. status [B] int32 bits:
 *   1 fewer than 4 masked pixels / fewer than `sample` points, 2 no consensus, 4 a candidate focal non-finite or not positive, 8 tables
 *   do not fit the image. info [B][C][4] int32: RANSAC iterations run, index of the chosen hypothesis (-1: none), sub-sample inliers
 *   after the refit, inliers over all n masked pixels.
 * workspace: geo4d_pnp_ransac_workspace bytes (0 for arguments the solver rejects), 8-byte aligned. Six launches, no allocation, no
 * synchronisation; fp64 with fixed-order reductions (deterministic). */
size_t geo4d_pnp_ransac_workspace(int B, int C, int H, int W, int iterations, int max_points);
int geo4d_pnp_ransac(const float* points, long image_stride, const float* conf, long conf_stride, float thr, const double* cand_focals,
                     double ppx, double ppy, double reproj, int iterations, int sample, const int* n, const int* m, const int* sub,
                     const int* draws, int max_points, int B, int C, int H, int W, double* focal, double* c2w, int* status, int* info,
                     void* workspace, size_t workspace_bytes, void* stream);

const char* geo4d_last_error(void);
int geo4d_abi_version(void);
/* sizeof of the parameter structs as the LIBRARY was compiled (which: 0 conv_gemm, 1 groupnorm, 2 attention, 3 align, 4 align_small; else 0):
 * bindings compare it with their own layout at load time. */
size_t geo4d_abi_struct_size(int which);

#ifdef __cplusplus
}
#endif
#endif
