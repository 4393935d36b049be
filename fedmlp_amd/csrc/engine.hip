// FedMLP engine: ResNet-18 and EfficientNet-B0 training/eval graphs over the HIP kernels + the
// C ABI of include/fedmlp_hip.h.  Host code only (kernels live in igemm/wgrad/elementwise/
// heads/effnet.hip).  One engine per process/GPU.
//
// Data layout in HBM (all fp32):
//   state   : [conv weights OHWI (stem padded to [64][7][8][4])][fc.W][fc.b][pad]
//             [gamma of all 20 BN][beta of all 20 BN] | [running_mean all][running_var all]
//             `- trainable (Adam, grads mirror this part) -'   `- FedAvg'd, not trained -'
//   activations NHWC; train-mode forward keeps per conv the raw output y, per block
//   the post-BN/ReLU z1 and the block output; the two views of a FedMLP step are
//   one batch of 2B images with per-view ("group") BN statistics.
//   EfficientNet-B0 (model 1): channel counts are padded to multiples of 16 inside the engine
//   (24->32, 40->48; padded weights/gamma/beta are 0 and stay 0 under Adam, so padded channels
//   carry exact zeros); depthwise weights are [k*k][C]; squeeze-excite W1 [Cs][C], W2 kept transposed [Cs][C].
//   Padded slots of the gradient arenas hold exact zeros too (the stem's zero taps are masked, a padded channel's activation
//   and gamma are 0, alignment gaps are never written), so SGD / AdamW keep the padding at 0 and the gradient norm may run over
//   the whole arena.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/fedmlp_hip.h"
#include "../../include/fedmlp_hip_debug.h"
#include "../../include/fedmlp_hip_rofl.h"
#include "../../include/fedmlp_hip_drift.h"
#include "../../include/fedmlp_hip_server.h"
#include "comm.h"
#include "common.h"
#include "kernels.h"
#include "pwconv.h"

static thread_local std::string g_err;
const char* fm_last_error(void) { return g_err.c_str(); }
const char* fm_version(void) { return "fedmlp_hip 0.2 (gfx950)"; }

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            char b_[512];                                                                      \
            snprintf(b_, sizeof b_, "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            g_err = b_;                                                                        \
            return FM_ERR_HIP;                                                                 \
        }                                                                                      \
    } while (0)
#define ARGCHK(c, msg)                                                       \
    do {                                                                     \
        if (!(c)) { g_err = std::string("bad argument: ") + msg; return FM_ERR_ARG; } \
    } while (0)
// refuse with what a `*_bad` validator answers (nullptr: fine)
#define BADCHK(x)                                                            \
    do {                                                                     \
        if (const char* bad_ = (x)) ARGCHK(false, bad_);                     \
    } while (0)

namespace {

struct DgradClass {
    TapList taps;
    int dh[9], dw[9];
    int ph, pw;
    int nsteps;
    float* wpack = nullptr;
    long long pl_off = -1;    // bf16 planes of wpack inside fm_engine::wpl_d (2-byte units), -1 = none
};

struct Conv {
    int cin, cout, k, stride, pad;
    int cin_p, kw_p;          // padded input channels / kernel width of the engine layout
    bool stem3 = false;       // ResNet's 7x7 stem, packed: K = 7 rows x (8 taps x 3 channels) + 8 zeros = 176 (engine.hip add_conv)
    int Hp = 0, Wp = 0;       // stem3: framed input sizes (hin + 6, win + 8)
    int cout_p;               // rows of the engine weight matrix (= cout for ResNet, padded to 16 for EfficientNet)
    int hin, win, hout, wout;
    size_t w_off;             // offset into the state arena
    size_t w_numel;           // cout_p*k*kw_p*cin_p
    int Kw;                   // k*kw_p*cin_p  (GEMM K of fwd, N of wgrad)
    int nsteps;               // Kw/16 (igemm K steps)
    int4* tab = nullptr;      // [Kw/4]
    int ncls = 0;
    DgradClass cls[4];
    int bn;                   // index of the BatchNorm that follows
    long long pl_off = -1;    // bf16 planes of the forward weights inside Weights::wpl_f (2-byte units), -1 = none
    long long wb_off = -1, wbt_off = -1;   // bf16 shadow of a 1x1 conv's weights [cout_p][cin_p] / transposed (bf16 mode)
    double macs_per_img;      // algorithmic MACs (real k, real cin)
    float* y = nullptr;       // raw conv output (train) [max_images][hout][wout][cout]
};

struct Bn {
    int C;                    // engine channels (padded)
    int C_real;               // state_dict channels
    int ch_off;               // channel offset inside the all-BN vectors
    float *mean, *istd, *scale, *shift;   // [2][C] train-mode per-group
};

struct Block { int c1, c2, ds; };      // ResNet basic block: conv indices (ds = -1: no downsample)

struct MBConv {               // EfficientNet block (efficientnet-pytorch MBConvBlock)
    int k, s, expand, cin, cout, cin_p, ce, ce_p, cout_p, cs;
    int hin, win, hout, wout, pad_t, pad_l;
    bool skip;
    int c_exp = -1, c_proj = -1;          // 1x1 conv indices
    int bn0 = -1, bn1 = -1, bn2 = -1;
    size_t dw_off, w1_off, b1_off, w2_off, b2_off;
};

// Where a launch goes: a stream and the workspaces only one stream may use at a time.  The engine has two: `main` (the caller's
// stream) and `side` (teacher forward, weight gradients; st == null in stream mode 1).
struct Lane {
    hipStream_t st = nullptr;
    float* sk_slab = nullptr;         // stream-K fix-up workspace of the conv GEMMs [blocks][2][BM*BN]
    int* sk_counters = nullptr;
    float* ws_slab = nullptr;         // partial slabs of the weight gradients (side: stream mode 0 only)
    // per-block records of the depthwise kernels (BN partial sums; the eval forward's pooling sums).  The main lane's IS its
    // ws_slab (no weight gradient runs on a lane while a depthwise conv does); the side lane has 64 MB of its own, since its
    // ws_slab exists only when the weight gradients run there
    float* rec = nullptr;
};

// One net's parameters and everything derived from them; two instances, student and teacher (fm_teacher_swap exchanges them)
struct Weights {
    float* state = nullptr;               // the state arena (layout at the top of this file)
    std::vector<int64_t> counters;        // num_batches_tracked per BN
    // Both flags are raised by net_changed() alone and travel with the copies they guard (fm_teacher_swap)
    float *ev_scale = nullptr, *ev_shift = nullptr;   // eval-mode BN affine of every channel, remade when ev_dirty (ensure_eval_affine)
    bool ev_dirty = true;
    // forward shadows, remade when fwd_dirty (ensure_fwd_shadows): bf16 W and W^T of the 1x1 convs (bf16 mode); bf16 planes of the
    // conv weights (ResNet; block-major in planes mode, pconv.hip, else row-major, split3.h); the stem's planes (stem_rows.hip)
    bf16* wb = nullptr;
    unsigned short *wpl_f = nullptr, *wst = nullptr;
    bool fwd_dirty = true;
};

// The tensors a forward writes.  The student's set is what the backward reads; the second set (fm_engine::tacts) exists only
// with the side stream, for the teacher's eval forward next to the student's train forward.
// A tensor that exists as fp32, as block-major bf16 planes (planes mode: what the conv GEMMs read), or both; a form that does not
// exist is null.  In: an operand a launcher reads; Out: one it writes, and whatever holds the buffers.  Planes nobody produced
// (In::p null where a planes kernel runs: test hooks) are made by scratch_planes.
struct In { const float* f = nullptr; const unsigned short* p = nullptr; };
struct Out {
    float* f = nullptr; unsigned short* p = nullptr;
    operator In() const { return {f, p}; }
};
// The form the graphs keep a block tensor in: planes only where it has planes (its fp32 buffer then idles: fm_debug_activation
// and the last block's residual re-form fp32 values into it), fp32 otherwise
inline Out kept(Out t) { return t.p ? Out{nullptr, t.p} : t; }

struct BlockActs {
    Out z1, out;
    float* ds_y = nullptr;            // the downsample conv's output (student: that Conv::y)
};
struct MBActs { float *a_e = nullptr, *y_d = nullptr, *a_s = nullptr, *out = nullptr, *sq = nullptr, *rpre = nullptr, *gate = nullptr; };
struct Acts {
    // ResNet-18: the stem's raw output (student: convs[0].y) and its pooled output (planes mode: written both ways)
    float* stem_y = nullptr;
    Out p0;
    float* a0 = nullptr;              // EfficientNet: swish(bn(stem))
    std::vector<BlockActs> blk;
    std::vector<MBActs> mb;
    float *T_mid = nullptr, *se_pool = nullptr;   // EfficientNet: head activation; squeeze-excite pooling partials
};

// BatchNorm mode of a train-mode forward: batch statistics; the same without touching running statistics and counters
// (fm_forward_recompute); every BatchNorm on its running statistics (fm_bn_freeze)
enum class BnMode { Batch, BatchNoUpdate, Frozen };
// what a backward is asked for beyond e->grad from e->dlogits
struct Bwd {
    bool frozen = false;              // the forward ran on frozen statistics: every BatchNorm-backward finalize takes its frozen form
    const float* dfeat = nullptr;     // d loss / d feature (caller-owned, or null)
    float* dx[2] = {nullptr, nullptr};    // where d loss / d image of the views goes (null = not wanted: no launch)
    bool step = true;                 // optimizer.step() at the end
    // per-layer requires_grad (fm_set_trainable): one flag per state entry in reference key order, null = every parameter.
    // The backward stops behind the first unit (forward order) that has a trainable parameter unless dx is wanted, and inside
    // the part that runs a frozen conv's weight gradient is not launched where it is a launch of its own.  e->grad then holds
    // stale values at the frozen entries: the caller masks them (fm_backward_grads_x: k_grad_accumulate_masked)
    const int32_t* train = nullptr;
};

// The gradient tensors a backward's weight gradients read, one set per block parity (fm_engine::rg / eg): with the weight gradients
// on the side lane (side_w) the two sets are buffers of their own, otherwise set [1] IS set [0] (alloc_workspaces / alloc_side)
struct ResGrads { Out dy2, dyd, dy1; };       // ResNet-18: d y2, d y_ds, d y1 (planes mode: the planes are what the GEMMs read)
struct EffGrads { float *dyp = nullptr, *dyd = nullptr, *dye = nullptr, *se_dg = nullptr, *se_dr = nullptr; };   // EfficientNet-B0: d y_p, d y_d, d y_e; the SE vectors

struct StateEntry {           // one state_dict entry, in reference key order
    int kind;                 // 0 OIHW weight (re-laid out to O,H,W(pad),I(pad)), 1 float vector, 2 int64 counter
    int conv;                 // conv index (kind 0, -1 for depthwise / squeeze-excite weights)
    size_t eng_off;           // engine arena offset
    size_t n;                 // elements in state_dict form
    int bn;                   // counter's BN index (kind 2)
    int O = 0, I = 0, KH = 0, KW = 0, Wpad = 0, Ipad = 0;   // kind 0 geometry
    int Ostride = 0;          // engine row stride when it exceeds KH*Wpad*Ipad (packed stem: 176), 0 = dense
    // the entry's span in the arena: a conv weight's O rows of `dense` floats, `row` apart, the last row ending with its matrix; a
    // vector's n elements as one row
    using Span = ArenaSpan;
    Span span() const
    {
        if (kind != 0) return {(int)n, (int)n, (long long)n};
        const int dense = KH * Wpad * Ipad, row = Ostride ? Ostride : dense;
        return {dense, row, (long long)(O - 1) * row + dense};
    }
};

// The entry / chunk table of the state arena (arena_table.h), a property of the model: built and uploaded once by fm_create
// (build_arena_table).  ent / chunks / ent_of / n_param_chunks are the host copy, d_ent / d_chunks the device arrays; ent_at maps
// an arena offset to the state entry (parameter) that starts there
struct ArenaTable : ArenaTableHost {
    ArenaEntry* d_ent = nullptr;
    ArenaChunk* d_chunks = nullptr;
    std::unordered_map<size_t, int> ent_at;
};

struct EvPair { hipEvent_t a, b; int family; double flops; };
struct OpEv { hipEvent_t a, b; int id; };
// a batched kernel's job table on the device (upload_jobs): the jobs, their count and the blocks of the one launch
template <typename J>
struct JobList { J* jobs = nullptr; int n = 0, blocks = 0; };

}  // namespace

struct fm_engine {
    fm_config cfg;
    Lane main, side;
    Weights student, teacher;
    Acts acts, tacts;
    int C = 0, D = 512, H = 0, W = 0, maxB = 0;
    std::vector<Conv> convs;
    std::vector<Bn> bns;
    std::vector<Block> blocks;
    std::vector<MBConv> mbs;
    int model = 0, c_stem = 0, c_head = -1, bn_stem = 0, bn_head = -1;
    float bn_eps = 1e-5f, bn_mom = 0.1f;
    int maxC = 512;                   // widest BN (sizes ca/cb/cc and the partial-sum workspace)
    ResGrads rg[2];                   // the backward's gradient sets by block parity (set [0]'s d y_d of EfficientNet-B0 is acts.T_mid)
    EffGrads eg[2];
    float *se_ds = nullptr, *hfeat = nullptr;
    const float *dc_dev = nullptr, *drop_dev = nullptr;   // caller-owned stochastic multipliers (or null)
    int pending_views = 0, pending_B = 0;                 // fm_forward_train awaiting fm_backward_step
    // autograd path (fm_backward_grads / fm_adam_step): the gradient accumulator (NP floats, allocated on first use; `gacc_full`
    // false = empty, the next backward copies)
    float* gacc = nullptr;
    bool gacc_full = false;
    // fm_grad_norm / fm_clip_grad_norm: the per-block partial sums of squares and the norm word of a call that gives no pointer
    // (allocated on first use)
    double* norm_part = nullptr;
    float* norm_word = nullptr;
    ArenaTable tab;                   // the entry / chunk table every chunked kernel walks
    double* dist_part = nullptr;      // fm_state_dist: the per-(chunk, k) partial sums (allocated on first use)
    uint8_t* strong_ws = nullptr;     // fm_augment_strong's uint8 images and LUTs for maxB samples, allocated on first use
    uint8_t* metrics_ws = nullptr;    // fm_eval_metrics' workspace (class-major scores, chunk counts, partials): grows on demand
    size_t metrics_ws_bytes = 0;
    // frozen BatchNorm statistics (fm_bn_freeze): `bn_freeze` is the handle flag fm_forward_train / fm_forward_recompute read,
    // `pending_fixed` the mode of the pending forward (its backward takes the same)
    bool bn_freeze = false, pending_fixed = false;
    // per-layer requires_grad and optimizer parameter groups (autograd path only).  `trainable`: one flag per state entry,
    // EMPTY = the default mask (every parameter trainable: every code path is then the one it was before masks existed);
    // `pending_trainable` the mask of the pending forward (its backward takes that one, like pending_fixed).  `group_of`: the
    // parameter group of each state entry, -1 = not optimized (fm_optim_groups; empty = no table).  Both are carried to the
    // kernels over `tab`'s parameter chunks as a selector (group_sel / mask_sel)
    std::vector<int32_t> trainable, pending_trainable, group_of;
    int n_groups = 0;
    std::vector<StateEntry> entries;
    int n_bn_ch = 0;
    size_t NP = 0, NS = 0;            // trainable floats (padded to 4), whole state floats
    size_t off_fcw = 0, off_fcb = 0, off_gamma = 0, off_beta = 0, off_rm = 0, off_rv = 0;
    int64_t nf_sd = 0, ni_sd = 0;     // state_dict sizes
    float *grad = nullptr, *adam_m = nullptr, *adam_v = nullptr;      // student only, like the data-gradient packs below
    float* stage_sd = nullptr;        // device staging buffer in state_dict order
    fm_adam hp{3e-5f, 0.9f, 0.999f, 1e-8f, 5e-4f};
    int64_t adam_t = 0;
    // workspaces
    float *x4 = nullptr, *dyh0 = nullptr;
    float* x3 = nullptr;      // packed stem: zero-framed NHWC3 input [max_images][H + 6][W + 8][3]
    // planes mode at 112-pixel stem rows (stem_rows.hip): the framed input as bf16 planes of four channels per pixel
    // [3][max_images][H + 6][W + 8][4] (the stem's weight planes [7][3][64][32] are Weights::wst)
    bool stem_rows = false;
    unsigned short* x3p = nullptr;
    long long x3p_plane_elems = 0;
    uint8_t* idx0 = nullptr;
    float *GA = nullptr, *GB = nullptr, *GE = nullptr;      // block input / output gradients (GB: EfficientNet-B0, GE: ResNet-18)
    float *ws_stats = nullptr, *ws_part = nullptr;
    // what ws_stats holds: the BN partial sums of conv `stats_conv`, `stats_tiles_n` tiles per group -- written by the conv_fwd
    // that launched the GEMM (the count depends on the kernel and on that call's operand prologue), read by the finalize
    int stats_conv = -1, stats_tiles_n = 0;
    size_t slab_floats = 0;
    float *ca = nullptr, *cb = nullptr, *cc = nullptr;
    float *feat = nullptr, *logits = nullptr, *tfeat = nullptr, *tlogits = nullptr, *dlogits = nullptr;
    // prototypes
    float* psum = nullptr;
    int64_t *pcnt = nullptr, *tcnt = nullptr;
    float* zeros = nullptr;
    int *sel_counts = nullptr, *sel_top = nullptr, *sel_bot = nullptr, *cls_dev = nullptr;
    int sel_cap = 0;
    // fm_loss_rofl / fm_step_rofl workspaces for max_images rows, allocated at the first RoFL call (rofl_ws)
    double *rofl_rowloss = nullptr, *rofl_dist = nullptr;
    float* rofl_cos = nullptr;
    int* rofl_keep = nullptr;
    // client-drift correction (fm_drift_begin .. fm_drift_end, include/fedmlp_hip_drift.h): while `drift_on`, every optimizer
    // step reads drift_gcorr, written by one launch in front of it (drift_grad), in place of its gradient.  NP floats each,
    // allocated by the first install that needs them: the anchor (the student's parameters at begin) and the corrected gradient
    // always, the shift with a shift, the running sum of raw gradients with track.  drift_steps: optimizer steps since begin
    bool drift_on = false, drift_shifted = false, drift_track = false;
    float drift_mu = 0.f;
    int64_t drift_steps = 0;
    float *drift_anchor = nullptr, *drift_shift = nullptr, *drift_gsum = nullptr, *drift_gcorr = nullptr;
    // server optimizer (fm_server_opt_begin .. fm_server_opt_end, include/fedmlp_hip_server.h): while `srv_on`, fm_server_opt_step
    // -- and nothing else -- enqueues server_opt.hip's launch.  The two moments are NP floats each, allocated by the first install
    // (v by the first adaptive one), like srv_part, one fp64 partial per parameter chunk of `tab`; srv_omb1 / srv_omb2 =
    // 1.0f - beta in fp32
    bool srv_on = false;
    fm_server_opt srv_hp{};
    float srv_omb1 = 0.f, srv_omb2 = 0.f;
    int64_t srv_steps = 0;
    float *srv_m = nullptr, *srv_v = nullptr;
    double* srv_part = nullptr;
    int* tag_buf = nullptr;           // fm_select_topk_rows: [pool sizes ncls | counts 2 ncls | top ncls*cap | bot ncls*cap | rows ncls*stride]
    size_t tag_buf_ints = 0;
    // profiling
    bool prof = false, prof_fail = false;
    hipError_t soft_err = hipSuccess;      // first failed event record / stream wait of the current step (soft())
    // a kernel's own failure report (pconv.hip: a stream-K part that never arrived): dev_err is read by the optimizer kernel
    // (the step does not touch the weights), host_err is its host-mapped twin that STEP_DONE checks at every call
    int* dev_err = nullptr;
    int* host_err = nullptr;
    int* host_err_dev = nullptr;
    // per-op timing (FM profile leg of tools/op_profile.py): label = "<op>@<block>"
    bool oprof = false;
    int ctx = -1;
    std::vector<std::string> op_names;
    std::vector<double> op_ms;
    std::vector<int64_t> op_n;
    std::vector<OpEv> opevs;
    std::vector<EvPair> evs;
    std::vector<hipEvent_t> ev_free;
    double prof_ms[FM_PROFILE_FAMILIES] = {}, prof_flops[FM_PROFILE_FAMILIES] = {};
    int64_t prof_n[FM_PROFILE_FAMILIES] = {};
    std::vector<void*> allocs;
    // The copies only the student has, raised by student_copies_stale() alone.  dgrad_dirty (remade by ensure_packed): the
    // transposed weight packs of the data gradients (DgradClass::wpack), rebuilt by ONE launch after every optimizer step (and
    // lazily after any other change of the state), and their bf16 planes wpl_d for the split-product GEMMs (ResNet, fp32 mode;
    // layout as Weights::wpl_f).  stem_dpack_stale (ensure_stem_dpack): ResNet-18's stem weights as its data gradient's B matrix
    // (stem_dgrad.hip), made on first use
    JobList<PackJob> pack_jobs;
    unsigned short* wpl_d = nullptr;
    bool dgrad_dirty = true;
    float* stem_dpack = nullptr;
    bool stem_dpack_stale = true;
    JobList<SplitJob> split_f, split_d;         // the plane jobs of the forward weights (either net's) / of the packs
    // planes mode (ResNet-18, split product forms): the 3x3 / 1x1 conv GEMMs take BOTH operands as block-major bf16 planes
    // (pconv.hip); the activation planes are written by the kernels that produce the tensors
    bool planes = false;
    unsigned short* xp_scratch = nullptr;       // planes of an fp32 operand nobody produced planes for (test hooks)
    unsigned short* xp_scratch2 = nullptr;      // ... and of the second operand of a weight gradient
    size_t xp_scratch_elems = 0;
    const float* xp_scratch_src = nullptr;
    long long xp_scratch_npix = 0;
    // RCCL (comm.hip)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    double* comm_buf = nullptr;       // device scratch of the small all-reduces
    size_t comm_buf_n = 0;
    int precision = 0;                // 0 fp32 activations, 1 bf16 activations (EfficientNet-B0 only)
    int products = 6;                 // fm_config.reserved[2]: how the fp32 conv GEMMs form their products (0 fp32 pipe, 6 / 9 bf16 partials)
    int stream_mode = 0;              // fm_config.reserved[1]: 0 side stream for teacher + weight gradients, 1 one stream, 2 teacher only
    int dt = DT_F32;                  // storage type of activations / their gradients (DT_F32 or DT_BF16)
    size_t wb_numel = 0;              // elements of Weights::wb
    JobList<CastJob> cast_jobs;
    bool fuse_gate = false;           // squeeze-excite gate applied on the project conv's operand load (a_s never stored)
    // stage-1 steps: the frozen teacher's forward is independent of the student's until the loss, so it is enqueued on the
    // side lane into the second activation set (side_ok; stream_mode 1: main lane, the student's set)
    hipEvent_t ev_in = nullptr, ev_t = nullptr;
    bool side_ok = false;
    // first image of the input staging (e->x4 / x3 / x3p / stem_col) the stem's FORWARD reads: 0, except while fm_step_rscfed
    // enqueues its teacher's forward, whose view is the staging's second group
    int in_img0 = 0;
    // backward: the weight gradients run on the side lane next to the data-gradient chain; the gradient tensors they read
    // (rg / eg) are double-buffered by block parity (side_w; stream_mode 1 or 2: inline)
    bool side_w = false;
    hipEvent_t ev_p[4][2] = {}, ev_c[4][2] = {}, ev_wdone = nullptr;    // [tensor: d y_p, d y_d, d y_e, SE vectors][block parity]
    float* stem_col = nullptr;        // bf16 mode: [images][hout][wout][k][4][4] bf16 im2col of the input (the stem's X operand)
    // Lane-order test hooks (fm_debug_lane_delay, fm_debug_drop_wait; fedmlp_hip_debug.h).  armed: the delay points count and the
    // `at`-th one of `lane` enqueues the delay kernel once; drop: bit k skips the cross-lane wait of kind k (lane_wait)
    struct LaneDbg {
        bool armed = false, fired = false;
        int lane = 0, micros = 0;
        int64_t at = 0, ticks = 0;
        int64_t points[2] = {0, 0};
        uint32_t drop = 0;
        int64_t waits[FM_WAIT_KINDS] = {}, skipped[FM_WAIT_KINDS] = {};
    } ldbg;
};
// a delay point of lane 0 (main) / 1 (side): see fm_debug_lane_delay
static void lane_point_armed(fm_engine* e, int lane);
static inline void lane_point(fm_engine* e, int lane)
{
    if (e->ldbg.armed) lane_point_armed(e, lane);
}
// Every cross-lane hipStreamWaitEvent of the lane protocol goes through here, so that fm_debug_drop_wait can leave one kind out
static inline hipError_t lane_wait(fm_engine* e, int kind, hipStream_t st, hipEvent_t ev)
{
    fm_engine::LaneDbg& d = e->ldbg;
    d.waits[kind] += 1;
    if (d.drop >> kind & 1) { d.skipped[kind] += 1; return hipSuccess; }
    return hipStreamWaitEvent(st, ev, 0);
}
static inline void soft(fm_engine* e, hipError_t rc)
{
    if (rc != hipSuccess && e->soft_err == hipSuccess) e->soft_err = rc;
}
// end of a step's launch sequence: a failed launch (hipGetLastError) or a failed cross-stream event operation surfaces here
#define STEP_DONE(e)                                                 \
    do {                                                             \
        const hipError_t se_ = (e)->soft_err;                        \
        (e)->soft_err = hipSuccess;                                  \
        HIPCHK(se_);                                                 \
        HIPCHK(hipGetLastError());                                   \
        if ((e)->host_err && *(volatile int*)(e)->host_err) {        \
            /* drain the failed step (its later kernels may report too), then clear both words: it is reported ONCE */ \
            (void)hipStreamSynchronize((e)->main.st);                \
            if ((e)->side.st) (void)hipStreamSynchronize((e)->side.st); \
            *(volatile int*)(e)->host_err = 0;                       \
            (void)hipMemsetAsync((e)->dev_err, 0, sizeof(int), (e)->main.st); \
            g_err = "a stream-K part never arrived (pconv): the step's optimizer update was skipped"; \
            return FM_ERR_HIP;                                       \
        }                                                            \
    } while (0)


namespace {

template <typename T>
int dalloc(fm_engine* e, T** p, size_t n)
{
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    e->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return FM_OK;
}
// pass a callee's failure on
#define RCCHK(x)                                       \
    do {                                               \
        const int rc_ = (x);                           \
        if (rc_ != FM_OK) return rc_;                  \
    } while (0)
#define DALLOC(p, n) RCCHK(dalloc(e, &(p), (n)))

// activation buffer of n elements in the engine's storage type (kept behind float* handles)
int aalloc(fm_engine* e, float** p, size_t n) { return dalloc(e, p, e->precision ? (n + 1) / 2 : n); }
#define AALLOC(p, n) RCCHK(aalloc(e, &(p), (n)))

// The engine's side stream runs at the LOWEST priority: the caller's stream carries the dependent chain (student forward,
// BatchNorm / data-gradient chain) whose short bandwidth-bound kernels should be dispatched first; the side stream's
// teacher forward / weight gradients fill what is left (ResNet-18 stage-1 step 37.7 -> 37.1 ms; highest priority: 38.3)
hipError_t create_side_stream(hipStream_t* st)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, least);
}

int upload_tab(fm_engine* e, const std::vector<int4>& h, int4** d)
{
    DALLOC(*d, h.size());
    HIPCHK(hipMemcpy(*d, h.data(), h.size() * sizeof(int4), hipMemcpyHostToDevice));
    return FM_OK;
}
template <typename J>
int upload_jobs(fm_engine* e, const std::vector<J>& h, int blocks, JobList<J>& d)
{
    d.n = (int)h.size(); d.blocks = blocks;
    DALLOC(d.jobs, h.size());
    if (!h.empty()) HIPCHK(hipMemcpy(d.jobs, h.data(), h.size() * sizeof(J), hipMemcpyHostToDevice));
    return FM_OK;
}

// ---- model construction -------------------------------------------------------
int add_conv(fm_engine* e, int cin, int cout, int k, int stride, int pad, int hin, int win, size_t& off)
{
    Conv c{};
    c.cin = cin; c.cout = cout; c.k = k; c.stride = stride; c.pad = pad;
    const bool eff = e->model == 1;
    c.cin_p = (cin == 3) ? 4 : (eff ? (cin + 15) / 16 * 16 : cin);
    c.cout_p = eff ? (cout + 15) / 16 * 16 : cout;
    c.kw_p = (cin == 3) ? (k <= 4 ? 4 : 8) : k;
    c.hin = hin; c.win = win;
    if (eff) {                       // TF-"same": out = ceil(in/stride); pad here = top/left padding
        c.hout = (hin + stride - 1) / stride;
        c.wout = (win + stride - 1) / stride;
    } else {
        c.hout = (hin + 2 * pad - k) / stride + 1;
        c.wout = (win + 2 * pad - k) / stride + 1;
    }
    c.Kw = k * c.kw_p * c.cin_p;
    const char* pk = getenv("FM_STEM_PACKED");
    if (cin == 3 && k == 7 && !eff && !(pk && atoi(pk) == 0)) {
        // packed 7x7 stem: a kernel row is the 24 contiguous floats (7 taps x 3 channels + one zero tap) of an NHWC3 row
        // of the zero-framed input; 7 x 24 = 168 -> 176 = 11 K-steps of 16 (the [7][8][4] form, FM_STEM_PACKED=0,
        // needs 14 and wastes 43 % of the weight gradient's tile columns)
        c.stem3 = true;
        c.cin_p = 3; c.kw_p = 8;
        c.Kw = 176;
        c.Hp = hin + 6; c.Wp = win + 8;
    }
    c.nsteps = c.Kw / 16;
    c.w_numel = (size_t)c.cout_p * c.Kw;
    c.w_off = off;
    off += c.w_numel;
    c.macs_per_img = (double)c.hout * c.wout * cout * cin * k * k;
    c.bn = (int)e->convs.size();
    e->convs.push_back(c);
    return (int)e->convs.size() - 1;
}

int build_tables(fm_engine* e)
{
    if (e->planes) {
        // planes mode needs every non-stem conv GEMM (forward and data gradient) inside pconv.hip's limits at max_images
        for (auto& c : e->convs) {
            if (c.cin == 3) continue;
            if (!pconv_takes(c.cout_p, c.cin_p, (long long)e->maxB * c.hin * c.win, c.win) ||
                !pconv_takes(c.cin_p, c.cout_p, (long long)e->maxB * c.hout * c.wout, c.wout) ||
                !pwgrad_takes(c.cout_p, c.cin_p, c.k, (long long)e->maxB * c.hout * c.wout, (long long)e->maxB * c.hin * c.win, c.win,
                              c.pad))
                e->planes = false;
        }
    }
    for (auto& c : e->convs) {
        if (c.Kw % 16 != 0) { g_err = "conv K not a multiple of 16"; return FM_ERR_ARG; }
        // forward / wgrad table: chunk q -> (kh, kw, ci0)
        std::vector<int4> t(c.Kw / 4);
        if (c.stem3) {                      // chunk q = floats 4j.. of kernel row kh's window at framed pixel (2 oh + kh, 2 ow)
            for (int q = 0; q < c.Kw / 4; ++q) t[q] = make_int4(q / 6, 0, 4 * (q % 6), q < 42 ? 1 : 0);
            RCCHK(upload_tab(e, t, &c.tab));
            continue;
        }
        for (int q = 0; q < c.Kw / 4; ++q) {
            const int n = 4 * q;
            const int tap = n / c.cin_p, ci0 = n % c.cin_p;
            const int kh = tap / c.kw_p, kw = tap % c.kw_p;
            t[q] = make_int4(kh - c.pad, kw - c.pad, ci0, kw < c.k ? 1 : 0);
        }
        RCCHK(upload_tab(e, t, &c.tab));
        if (c.cin == 3) continue;          // the stem's input gradient has its own kernels (stem_dgrad.hip)
        // data-gradient parity classes
        const int s = c.stride;
        for (int ph = 0; ph < s; ++ph)
            for (int pw = 0; pw < s; ++pw) {
                DgradClass d{};
                d.ph = ph; d.pw = pw; d.taps.n = 0;
                for (int kh = 0; kh < c.k; ++kh)
                    for (int kw = 0; kw < c.k; ++kw) {
                        if ((ph + c.pad - kh) % s != 0 || (pw + c.pad - kw) % s != 0) continue;
                        const int j = d.taps.n++;
                        d.taps.t[j] = kh * c.k + kw;
                        d.dh[j] = (ph + c.pad - kh) / s;     // exact (divisible), may be negative
                        d.dw[j] = (pw + c.pad - kw) / s;
                    }
                if (d.taps.n == 0) continue;
                const int K = d.taps.n * c.cout_p;
                d.nsteps = K / 16;
                DALLOC(d.wpack, (size_t)c.cin_p * K);
                c.cls[c.ncls++] = d;
            }
    }
    // one job per (conv, parity class) for the batched pack kernel
    std::vector<PackJob> jobs;
    int blk = 0;
    for (auto& c : e->convs)
        for (int k = 0; k < c.ncls; ++k) {
            const DgradClass& d = c.cls[k];
            PackJob j{};
            j.w_off = (long long)c.w_off; j.out = d.wpack; j.Co = c.cout_p; j.T = c.k * c.k; j.Ci = c.cin_p;
            j.ntaps = d.taps.n;
            for (int t = 0; t < d.taps.n; ++t) j.taps[t] = d.taps.t[t];
            j.blk0 = blk;
            blk += pack_job_blocks(c.cout_p, c.cin_p, d.taps.n);
            jobs.push_back(j);
        }
    if (e->precision) {        // bf16 shadows (W and W^T) of every 1x1 convolution
        std::vector<CastJob> cj;
        long long off = 0;
        int cb = 0;
        for (auto& c : e->convs) {
            const bool stem = c.cin == 3 && e->model == 1;    // the stem runs as a K = k*kw_p*4 pointwise conv on its im2col
            if (c.k != 1 && !stem) continue;
            const int Kc = stem ? c.Kw : c.cin_p;
            const long long n = (long long)c.cout_p * Kc;
            c.wb_off = off; c.wbt_off = off + n;
            cj.push_back({(long long)c.w_off, c.wb_off, c.wbt_off, c.cout_p, Kc, cb});
            off += 2 * n;
            cb += (int)((n + 255) / 256);
        }
        e->wb_numel = (size_t)off;
        RCCHK(upload_jobs(e, cj, cb, e->cast_jobs));
        DALLOC(e->student.wb, e->wb_numel); DALLOC(e->teacher.wb, e->wb_numel);
    }
    RCCHK(upload_jobs(e, jobs, blk, e->pack_jobs));
    if (e->model == 0 && !e->precision) {
        // bf16 planes of the weights (forward) and of the packs (data gradient) for the GEMMs with whole 64-row tiles and whole
        // 32-k blocks per tap: every non-stem conv of ResNet-18 and every parity class of its data gradients.  The jobs, sizes
        // and offsets are the same for both layouts; e->planes says which kernel fills them (ensure_fwd_shadows, ensure_packed)
        // and which GEMM reads them (pconv.hip: block-major; igemm.hip, WP form: row-major, read where the product form splits)
        std::vector<SplitJob> jf, jd;
        long long off_f = 0, off_d = 0;
        int bf = 0, bd = 0;
        for (auto& c : e->convs) {
            if (c.cin == 3) continue;
            if (c.cout_p % 64 == 0 && c.cin_p % 32 == 0) {
                c.pl_off = off_f;
                jf.push_back({(long long)c.w_off, nullptr, off_f, c.cout_p, c.k * c.k, c.cin_p / 32, bf});
                bf += split_job_blocks(c.cout_p, c.k * c.k, c.cin_p / 32);
                off_f += (long long)c.cout_p * c.Kw * 3;
            }
            if (c.cin_p % 64 == 0 && c.cout_p % 32 == 0)
                for (int k = 0; k < c.ncls; ++k) {
                    DgradClass& d = c.cls[k];
                    d.pl_off = off_d;
                    jd.push_back({0, d.wpack, off_d, c.cin_p, d.taps.n, c.cout_p / 32, bd});
                    bd += split_job_blocks(c.cin_p, d.taps.n, c.cout_p / 32);
                    off_d += (long long)c.cin_p * d.taps.n * c.cout_p * 3;
                }
        }
        float* tmp = nullptr;
        if (off_f) {
            DALLOC(tmp, (size_t)(off_f + 1) / 2); e->student.wpl_f = reinterpret_cast<unsigned short*>(tmp);
            DALLOC(tmp, (size_t)(off_f + 1) / 2); e->teacher.wpl_f = reinterpret_cast<unsigned short*>(tmp);
        }
        if (off_d) { DALLOC(tmp, (size_t)(off_d + 1) / 2); e->wpl_d = reinterpret_cast<unsigned short*>(tmp); }
        RCCHK(upload_jobs(e, jf, bf, e->split_f));
        RCCHK(upload_jobs(e, jd, bd, e->split_d));
    }
    return FM_OK;
}

int build_resnet18(fm_engine* e)
{
    size_t off = 0;
    int h = e->H, w = e->W;
    add_conv(e, 3, 64, 7, 2, 3, h, w, off);
    h /= 2; w /= 2;          // conv1
    h /= 2; w /= 2;          // maxpool
    int cin = 64;
    const int widths[4] = {64, 128, 256, 512};
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < 2; ++b) {
            const int wd = widths[li];
            const int stride = (li > 0 && b == 0) ? 2 : 1;
            Block blk{};
            blk.c1 = add_conv(e, cin, wd, 3, stride, 1, h, w, off);
            const int ho = e->convs[blk.c1].hout, wo = e->convs[blk.c1].wout;
            blk.c2 = add_conv(e, wd, wd, 3, 1, 1, ho, wo, off);
            blk.ds = (stride != 1 || cin != wd) ? add_conv(e, cin, wd, 1, stride, 0, h, w, off) : -1;
            e->blocks.push_back(blk);
            cin = wd; h = ho; w = wo;
        }
    e->off_fcw = off; off += (size_t)e->C * 512;
    e->off_fcb = off; off += e->C;
    off = (off + 3) & ~(size_t)3;
    int ch = 0;
    for (auto& c : e->convs) {
        Bn b{};
        b.C = c.cout; b.C_real = c.cout; b.ch_off = ch; ch += c.cout;
        e->bns.push_back(b);
    }
    e->n_bn_ch = ch;
    e->off_gamma = off; off += ch;
    e->off_beta = off; off += ch;
    e->NP = off;             // ch is a multiple of 64 -> NP multiple of 4
    e->off_rm = off; off += ch;
    e->off_rv = off; off += ch;
    e->NS = off;
    // state_dict entry table (torchvision key order)
    auto push_conv = [&](int ci) {
        const Conv& c = e->convs[ci];
        e->entries.push_back({0, ci, c.w_off, (size_t)c.cout * c.cin * c.k * c.k, -1, c.cout, c.cin, c.k, c.k, c.kw_p,
                              c.cin_p, c.stem3 ? c.Kw : 0});
    };
    auto push_bn = [&](int bi) {
        const Bn& b = e->bns[bi];
        e->entries.push_back({1, -1, e->off_gamma + b.ch_off, (size_t)b.C, -1});
        e->entries.push_back({1, -1, e->off_beta + b.ch_off, (size_t)b.C, -1});
        e->entries.push_back({1, -1, e->off_rm + b.ch_off, (size_t)b.C, -1});
        e->entries.push_back({1, -1, e->off_rv + b.ch_off, (size_t)b.C, -1});
        e->entries.push_back({2, -1, 0, 1, bi});
    };
    push_conv(0); push_bn(0);
    for (auto& blk : e->blocks) {
        push_conv(blk.c1); push_bn(blk.c1);
        push_conv(blk.c2); push_bn(blk.c2);
        if (blk.ds >= 0) { push_conv(blk.ds); push_bn(blk.ds); }
    }
    e->entries.push_back({1, -1, e->off_fcw, (size_t)e->C * 512, -1});
    e->entries.push_back({1, -1, e->off_fcb, (size_t)e->C, -1});
    e->nf_sd = 0; e->ni_sd = 0;
    for (auto& en : e->entries) (en.kind == 2 ? e->ni_sd : e->nf_sd) += (int64_t)en.n;
    e->student.counters.assign(e->bns.size(), 0);
    e->teacher.counters = e->student.counters;
    return FM_OK;
}

// EfficientNet-B0 (efficientnet-pytorch 0.7.1 'efficientnet-b0', width/depth 1.0): stem 3x3 s2 ->
// 16 MBConv blocks -> head 1x1 -> pool -> dropout -> fc.  State entries follow the package's
// state_dict order (fedmlp_amd/spec.py:efficientnet_b0_entries is the host-side mirror).
int build_effnet_b0(fm_engine* e)
{
    static const int stages[7][6] = {{1, 3, 1, 1, 32, 16},  {2, 3, 2, 6, 16, 24},  {2, 5, 2, 6, 24, 40},
                                     {3, 3, 2, 6, 40, 80},  {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192},
                                     {1, 3, 1, 6, 192, 320}};
    e->bn_eps = 1e-3f; e->bn_mom = 0.01f; e->D = 1280;
    auto r16 = [](int c) { return (c + 15) / 16 * 16; };
    size_t off = 0;
    int ch = 0;
    auto add_bn = [&](int c_real) {
        Bn b{};
        b.C = r16(c_real); b.C_real = c_real; b.ch_off = ch; ch += b.C;
        e->bns.push_back(b);
        return (int)e->bns.size() - 1;
    };
    auto same_pad = [](int size, int k, int s) {
        const int o = (size + s - 1) / s;
        const int p = std::max((o - 1) * s + k - size, 0);
        return p / 2;
    };
    int h = e->H, w = e->W;
    e->c_stem = add_conv(e, 3, 32, 3, 2, same_pad(h, 3, 2), h, w, off);
    e->bn_stem = add_bn(32);
    e->convs[e->c_stem].bn = e->bn_stem;
    h = e->convs[e->c_stem].hout; w = e->convs[e->c_stem].wout;
    for (int st = 0; st < 7; ++st)
        for (int r = 0; r < stages[st][0]; ++r) {
            MBConv m{};
            m.k = stages[st][1];
            m.s = r == 0 ? stages[st][2] : 1;
            m.expand = stages[st][3];
            m.cin = r == 0 ? stages[st][4] : stages[st][5];
            m.cout = stages[st][5];
            m.cin_p = r16(m.cin); m.ce = m.cin * m.expand; m.ce_p = r16(m.ce); m.cout_p = r16(m.cout);
            m.cs = std::max(1, m.cin / 4);
            m.hin = h; m.win = w;
            m.hout = (h + m.s - 1) / m.s; m.wout = (w + m.s - 1) / m.s;
            m.pad_t = same_pad(h, m.k, m.s); m.pad_l = same_pad(w, m.k, m.s);
            m.skip = m.s == 1 && m.cin == m.cout;
            if (m.expand != 1) {
                m.c_exp = add_conv(e, m.cin, m.ce, 1, 1, 0, h, w, off);
                m.bn0 = add_bn(m.ce);
                e->convs[m.c_exp].bn = m.bn0;
            }
            m.dw_off = off; off += (size_t)m.k * m.k * m.ce_p;
            m.bn1 = add_bn(m.ce);
            m.w1_off = off; off += (size_t)m.cs * m.ce_p;
            m.b1_off = off; off += (size_t)(m.cs + 3) / 4 * 4;
            m.w2_off = off; off += (size_t)m.ce_p * m.cs;
            m.b2_off = off; off += m.ce_p;
            off = (off + 3) & ~(size_t)3;
            m.c_proj = add_conv(e, m.ce, m.cout, 1, 1, 0, m.hout, m.wout, off);
            m.bn2 = add_bn(m.cout);
            e->convs[m.c_proj].bn = m.bn2;
            e->mbs.push_back(m);
            h = m.hout; w = m.wout;
        }
    e->c_head = add_conv(e, 320, 1280, 1, 1, 0, h, w, off);
    e->bn_head = add_bn(1280);
    e->convs[e->c_head].bn = e->bn_head;
    e->off_fcw = off; off += (size_t)e->C * 1280;
    e->off_fcb = off; off += e->C;
    off = (off + 3) & ~(size_t)3;
    e->n_bn_ch = ch;
    e->off_gamma = off; off += ch;
    e->off_beta = off; off += ch;
    e->NP = off;
    e->off_rm = off; off += ch;
    e->off_rv = off; off += ch;
    e->NS = off;
    e->maxC = 1280;
    // ---- state_dict entries ----------------------------------------------------------------
    auto push_conv = [&](int ci) {
        const Conv& c = e->convs[ci];
        e->entries.push_back({0, ci, c.w_off, (size_t)c.cout * c.cin * c.k * c.k, -1, c.cout, c.cin, c.k, c.k, c.kw_p,
                              c.cin_p});
    };
    auto push_bn = [&](int bi) {
        const Bn& b = e->bns[bi];
        e->entries.push_back({1, -1, e->off_gamma + b.ch_off, (size_t)b.C_real, -1});
        e->entries.push_back({1, -1, e->off_beta + b.ch_off, (size_t)b.C_real, -1});
        e->entries.push_back({1, -1, e->off_rm + b.ch_off, (size_t)b.C_real, -1});
        e->entries.push_back({1, -1, e->off_rv + b.ch_off, (size_t)b.C_real, -1});
        e->entries.push_back({2, -1, 0, 1, bi});
    };
    push_conv(e->c_stem); push_bn(e->bn_stem);
    for (auto& m : e->mbs) {
        if (m.c_exp >= 0) { push_conv(m.c_exp); push_bn(m.bn0); }
        // depthwise [ce][1][k][k] -> [k][k][ce_p]: an OIHW->OHWI re-layout with O=1, I=ce
        e->entries.push_back({0, -1, m.dw_off, (size_t)m.ce * m.k * m.k, -1, 1, m.ce, m.k, m.k, m.k, m.ce_p});
        push_bn(m.bn1);
        e->entries.push_back({0, -1, m.w1_off, (size_t)m.cs * m.ce, -1, m.cs, m.ce, 1, 1, 1, m.ce_p});
        e->entries.push_back({1, -1, m.b1_off, (size_t)m.cs, -1});
        // _se_expand.weight [ce][cs][1][1] is kept TRANSPOSED, [cs][ce_p] like W1 (every squeeze-excite kernel then reads both
        // matrices with the channel index on the lanes): an "OIHW" view O = 1, I = ce, H = cs, W = 1 -> [1][cs][1][ce_p]
        e->entries.push_back({0, -1, m.w2_off, (size_t)m.ce * m.cs, -1, 1, m.ce, m.cs, 1, 1, m.ce_p});
        e->entries.push_back({1, -1, m.b2_off, (size_t)m.ce, -1});
        push_conv(m.c_proj); push_bn(m.bn2);
    }
    push_conv(e->c_head); push_bn(e->bn_head);
    e->entries.push_back({1, -1, e->off_fcw, (size_t)e->C * 1280, -1});
    e->entries.push_back({1, -1, e->off_fcb, (size_t)e->C, -1});
    e->nf_sd = 0; e->ni_sd = 0;
    for (auto& en : e->entries) (en.kind == 2 ? e->ni_sd : e->nf_sd) += (int64_t)en.n;
    e->student.counters.assign(e->bns.size(), 0);
    e->teacher.counters = e->student.counters;
    return FM_OK;
}

// planes of `elems` fp32 values: 3 x 2 B each
int palloc(fm_engine* e, unsigned short** pp, size_t elems)
{
    float* t = nullptr;
    DALLOC(t, (elems * 3 + 1) / 2);
    *pp = reinterpret_cast<unsigned short*>(t);
    return FM_OK;
}
#define PALLOC(p, n) RCCHK(palloc(e, &(p), (n)))

// EfficientNet tensor sizes at max_images (elements): block input / output, d y_p, d y_d and the head, d y_e; widest ce / cs
struct EffSizes { size_t g_io = 0, t_small = 0, t_mid = 0, t_big = 0, max_ce = 0, max_cs = 0; };
EffSizes eff_sizes(const fm_engine* e)
{
    const size_t B = e->maxB;
    const Conv& c0 = e->convs[0];
    EffSizes z;
    z.g_io = B * c0.hout * c0.wout * c0.cout_p;
    for (auto& m : e->mbs) {
        const size_t nin = B * m.hin * m.win, nout = B * m.hout * m.wout;
        z.g_io = std::max(z.g_io, std::max(nin * m.cin_p, nout * m.cout_p));
        z.t_small = std::max(z.t_small, nout * m.cout_p);
        z.t_mid = std::max(z.t_mid, nout * m.ce_p);
        z.t_big = std::max(z.t_big, nin * m.ce_p);
        z.max_ce = std::max<size_t>(z.max_ce, m.ce_p); z.max_cs = std::max<size_t>(z.max_cs, m.cs);
    }
    const Conv& chd = e->convs[e->c_head];
    z.t_mid = std::max(z.t_mid, B * chd.hout * chd.wout * chd.cout_p);
    return z;
}

// One activation set.  `second`: the side lane's set for the teacher's eval forward, with its own stem / downsample outputs
// (the student's are the Conv::y the train forward writes) and pooling partials without the backward's five sums
int alloc_acts(fm_engine* e, Acts& a, bool second)
{
    const size_t B = e->maxB;
    const Conv& c0 = e->convs[0];
    if (e->model == 0) {
        const size_t pooled = B * (c0.hout / 2) * (c0.wout / 2) * 64;
        a.stem_y = c0.y;
        if (second) DALLOC(a.stem_y, B * c0.hout * c0.wout * c0.cout_p);
        DALLOC(a.p0.f, pooled);
        if (e->planes) PALLOC(a.p0.p, pooled);
        a.blk.resize(e->blocks.size());
        for (size_t i = 0; i < e->blocks.size(); ++i) {
            const Block& blk = e->blocks[i];
            BlockActs& ba = a.blk[i];
            const Conv& c = e->convs[blk.c1];
            const size_t n = B * c.hout * c.wout * c.cout;
            DALLOC(ba.z1.f, n); DALLOC(ba.out.f, n);
            if (blk.ds >= 0) {
                ba.ds_y = e->convs[blk.ds].y;
                if (second) DALLOC(ba.ds_y, n);
            }
            if (e->planes) { PALLOC(ba.z1.p, n); PALLOC(ba.out.p, n); }
        }
        return FM_OK;
    }
    const EffSizes z = eff_sizes(e);
    AALLOC(a.a0, B * c0.hout * c0.wout * c0.cout_p);
    a.mb.resize(e->mbs.size());
    for (size_t i = 0; i < e->mbs.size(); ++i) {
        const MBConv& m = e->mbs[i];
        MBActs& ma = a.mb[i];
        const size_t nin = B * m.hin * m.win, nout = B * m.hout * m.wout;
        if (m.c_exp >= 0) AALLOC(ma.a_e, nin * m.ce_p);
        AALLOC(ma.y_d, nout * m.ce_p); AALLOC(ma.a_s, nout * m.ce_p);
        AALLOC(ma.out, nout * m.cout_p);
        DALLOC(ma.sq, B * m.ce_p); DALLOC(ma.rpre, B * m.cs); DALLOC(ma.gate, B * m.ce_p);
    }
    AALLOC(a.T_mid, z.t_mid);
    DALLOC(a.se_pool, B * 16 * (second ? 1 : 5) * z.max_ce);       // [imgs][<=16 chunks][5 sums][C]
    return FM_OK;
}

size_t sk_floats() { return std::max((size_t)igemm_max_blocks() * 2 * 16384, pconv_slab_floats()); }   // [blocks][2][BM*BN]

// Would the side lane's buffers fit?  They roughly double the activation footprint: one stream is kept when they would not
// fit with 4 GB to spare (fm_stream_mode() reports the mode that was actually set up).  Asked at the point of alloc_workspaces
// where the model's second set used to be allocated, so that the answer is the one it has always been.
bool side_fits(const fm_engine* e)
{
    const size_t B = e->maxB;
    const Conv& c0 = e->convs[0];
    size_t need = 0, spare = 0, free_b = 0, total_b = 0;
    if (e->model == 0) {
        // the teacher's activation set, the second gradient / slab buffers
        const size_t pooled = B * (c0.hout / 2) * (c0.wout / 2) * 64;
        need = (B * c0.hout * c0.wout * c0.cout_p + 4 * pooled + e->slab_floats) * 4;
        for (auto& blk : e->blocks) {
            const Conv& c = e->convs[blk.c1];
            need += (size_t)(blk.ds >= 0 ? 3 : 2) * B * c.hout * c.wout * c.cout * 4;
        }
        need += sk_floats() * 4 + ((size_t)4 << 20);
        if (e->planes) need += need * 3 / 2;       // the planes of the teacher's activations and of the second gradient set
        spare = (size_t)4 << 30;
    } else {
        // next to what is still to be allocated (slabs, statistics: < 2 GB)
        const EffSizes z = eff_sizes(e);
        const size_t es = e->precision ? 2 : 4;
        for (auto& m : e->mbs) {
            const size_t nin = B * m.hin * m.win, nout = B * m.hout * m.wout;
            need += ((m.c_exp >= 0 ? nin * m.ce_p : 0) + 2 * nout * m.ce_p + nout * m.cout_p) * es;
        }
        need += (z.t_small + 2 * z.t_mid + z.t_big) * es + 2 * ((size_t)48 << 22);
        spare = (size_t)6 << 30;
    }
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= need + spare;
}

// The side lane and what runs on it: the teacher's activation set (stream mode 0 or 2) and, in stream mode 0, the second
// slab / gradient buffers of the weight gradients.
// ResNet-18 (MFMA-bound, persistent 512-block kernels): 39.0 -> 37.7 ms per stage-1 step with the teacher and the weight
// gradients on the side stream, same bits.  Co-running kernels stretch each other's launch windows, so per-kernel durations
// (bench.py's roofline, rocprofv3) are taken from a one-stream engine (stream mode 1).
int alloc_side(fm_engine* e)
{
    const size_t B = e->maxB;
    Lane& s = e->side;
    DALLOC(s.sk_slab, sk_floats());
    DALLOC(s.sk_counters, (size_t)1 << 20);
    HIPCHK(hipMemset(s.sk_counters, 0, ((size_t)1 << 20) * 4));
    RCCHK(alloc_acts(e, e->tacts, true));
    if (e->model == 1) DALLOC(s.rec, (size_t)16 << 20);           // pooling records of the eval depthwise forward (<= 33 MB)
    HIPCHK(create_side_stream(&s.st));
    HIPCHK(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->ev_t, hipEventDisableTiming));
    e->side_ok = true;
    if (e->stream_mode != 0) return FM_OK;
    DALLOC(s.ws_slab, e->slab_floats);
    if (e->model == 0) {
        const Conv& c0 = e->convs[0];
        const size_t pooled = B * (c0.hout / 2) * (c0.wout / 2) * 64;
        ResGrads& g = e->rg[1];
        DALLOC(g.dy2.f, pooled); DALLOC(g.dyd.f, pooled); DALLOC(g.dy1.f, pooled);
        if (e->planes) { PALLOC(g.dy2.p, pooled); PALLOC(g.dyd.p, pooled); PALLOC(g.dy1.p, pooled); }
    } else {
        const EffSizes z = eff_sizes(e);
        EffGrads& g = e->eg[1];
        AALLOC(g.dyp, z.t_small); AALLOC(g.dyd, z.t_mid); AALLOC(g.dye, z.t_big);
        DALLOC(g.se_dg, B * z.max_ce); DALLOC(g.se_dr, B * z.max_cs);
    }
    for (int k = 0; k < 4; ++k)
        for (int q = 0; q < 2; ++q) {
            HIPCHK(hipEventCreateWithFlags(&e->ev_p[k][q], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e->ev_c[k][q], hipEventDisableTiming));
        }
    HIPCHK(hipEventCreateWithFlags(&e->ev_wdone, hipEventDisableTiming));
    e->side_w = true;
    return FM_OK;
}

int alloc_workspaces(fm_engine* e)
{
    const size_t B = e->maxB;
    for (Weights* w : {&e->student, &e->teacher}) {
        DALLOC(w->state, e->NS);
        HIPCHK(hipMemset(w->state, 0, e->NS * 4));
        DALLOC(w->ev_scale, e->n_bn_ch); DALLOC(w->ev_shift, e->n_bn_ch);
    }
    DALLOC(e->grad, e->NP); DALLOC(e->adam_m, e->NP); DALLOC(e->adam_v, e->NP);
    HIPCHK(hipMemset(e->grad, 0, e->NP * 4));
    HIPCHK(hipMemset(e->adam_m, 0, e->NP * 4)); HIPCHK(hipMemset(e->adam_v, 0, e->NP * 4));
    DALLOC(e->stage_sd, (size_t)e->nf_sd);
    DALLOC(e->x4, B * e->H * e->W * 4);
    if (e->convs[0].stem3) {
        const size_t n3 = B * e->convs[0].Hp * e->convs[0].Wp * 3 + 64;      // + slack for the last window's over-read
        DALLOC(e->x3, n3);
        HIPCHK(hipMemset(e->x3, 0, n3 * 4));                                   // the frame stays zero for the engine's life
        const Conv& c0 = e->convs[0];
        e->x3p_plane_elems = (long long)B * c0.Hp * c0.Wp * 4;
        e->stem_rows = e->planes && stem_rows_takes(c0.k, c0.stride, c0.cout_p, c0.hout, c0.wout, e->x3p_plane_elems * 2);
        if (e->stem_rows) {
            DALLOC(e->x3p, (size_t)3 * e->x3p_plane_elems + 64);
            HIPCHK(hipMemset(e->x3p, 0, ((size_t)3 * e->x3p_plane_elems + 64) * 2));
            DALLOC(e->student.wst, 7 * 3 * 64 * 32); DALLOC(e->teacher.wst, 7 * 3 * 64 * 32);
        }
    }
    size_t max_stats = 0, max_slab = 0;
    for (auto& c : e->convs) {
        AALLOC(c.y, B * c.hout * c.wout * c.cout_p);
        if (c.cin == 3 && e->precision) AALLOC(e->stem_col, B * c.hout * c.wout * c.Kw);   // bf16 im2col of the input batch
        size_t tiles = (B * c.hout * c.wout + igemm_tile_n(c.cout_p, c.cin == 3) - 1) / igemm_tile_n(c.cout_p, c.cin == 3) + 2;
        if (e->precision) tiles = std::max<size_t>(tiles, B * c.hout * c.wout / 128 + 4);   // pw_blocks(): >= 128 pixels per block
        max_stats = std::max(max_stats, (tiles + 2 * 32) * 2 * c.cout_p);   // + folded partials
        max_slab = std::max(max_slab, c.w_numel);
    }
    for (auto& b : e->bns) {
        DALLOC(b.mean, 2 * b.C); DALLOC(b.istd, 2 * b.C); DALLOC(b.scale, 2 * b.C); DALLOC(b.shift, 2 * b.C);
    }
    RCCHK(alloc_acts(e, e->acts, false));
    bool side = e->stream_mode != 1;          // fm_config.reserved[1]: 0 two streams, 1 one stream, 2 teacher only
    const Conv& c0 = e->convs[0];
    if (e->model == 0) {
        const size_t pooled = B * (c0.hout / 2) * (c0.wout / 2) * 64;
        DALLOC(e->idx0, pooled);
        DALLOC(e->dyh0, B * c0.hout * c0.wout * 64);
        ResGrads& g = e->rg[0];
        DALLOC(e->GA, pooled); DALLOC(g.dy2.f, pooled); DALLOC(g.dyd.f, pooled); DALLOC(g.dy1.f, pooled); DALLOC(e->GE, pooled);
    } else {
        const EffSizes z = eff_sizes(e);
        AALLOC(e->GA, z.g_io); AALLOC(e->GB, z.g_io);
        EffGrads& g = e->eg[0];
        g.dyd = e->acts.T_mid;
        AALLOC(g.dyp, z.t_small); AALLOC(g.dye, z.t_big);
        DALLOC(g.se_dg, B * z.max_ce); DALLOC(g.se_dr, B * z.max_cs); DALLOC(e->se_ds, B * z.max_ce);
        side = side && side_fits(e);
        DALLOC(e->hfeat, B * e->D);
    }
    DALLOC(e->ws_stats, max_stats);
    DALLOC(e->ws_part, (size_t)2 * (1024 + 32) * 2 * e->maxC);   // per-block partials + folded partials
    e->slab_floats = std::max<size_t>(max_slab * 8, (size_t)48 << 20);   // >= 192 MB of partial slabs
    DALLOC(e->main.ws_slab, e->slab_floats);
    e->main.rec = e->main.ws_slab;
    DALLOC(e->ca, 2 * e->maxC); DALLOC(e->cb, 2 * e->maxC); DALLOC(e->cc, 2 * e->maxC);
    DALLOC(e->feat, B * e->D); DALLOC(e->tfeat, B * e->D);
    DALLOC(e->logits, B * e->C); DALLOC(e->tlogits, B * e->C); DALLOC(e->dlogits, B * e->C);
    DALLOC(e->psum, (size_t)2 * e->C * e->D); DALLOC(e->pcnt, 2 * e->C); DALLOC(e->tcnt, e->C);
    DALLOC(e->sel_counts, 2); DALLOC(e->cls_dev, FM_MAX_CLASSES);
    DALLOC(e->zeros, 64);
    if (e->planes) {
        const size_t pooled = B * (c0.hout / 2) * (c0.wout / 2) * 64;
        PALLOC(e->rg[0].dy2.p, pooled); PALLOC(e->rg[0].dyd.p, pooled); PALLOC(e->rg[0].dy1.p, pooled);
        // scratch planes for operands that arrive as fp32 (test hooks): the largest conv input / output-gradient tensor
        size_t mx = 0;
        for (auto& c : e->convs) {
            if (c.cin == 3) continue;
            mx = std::max(mx, std::max(B * c.hin * c.win * c.cin_p, B * c.hout * c.wout * c.cout_p));
        }
        e->xp_scratch_elems = mx * 3;
        float* t3 = nullptr;
        DALLOC(t3, (e->xp_scratch_elems + 1) / 2);
        e->xp_scratch = reinterpret_cast<unsigned short*>(t3);
        DALLOC(t3, (e->xp_scratch_elems + 1) / 2);
        e->xp_scratch2 = reinterpret_cast<unsigned short*>(t3);
    }
    DALLOC(e->main.sk_slab, sk_floats());
    DALLOC(e->dev_err, 16);
    HIPCHK(hipMemset(e->dev_err, 0, 16 * sizeof(int)));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&e->host_err), 64, hipHostMallocMapped));
    *e->host_err = 0;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&e->host_err_dev), e->host_err, 0));
    DALLOC(e->main.sk_counters, (size_t)1 << 20);
    HIPCHK(hipMemset(e->main.sk_counters, 0, ((size_t)1 << 20) * 4));
    HIPCHK(hipMemset(e->zeros, 0, 64 * 4));
    if (e->model == 0) side = side && side_fits(e);
    e->rg[1] = e->rg[0]; e->eg[1] = e->eg[0];       // one set for both parities, unless alloc_side gives the second its own buffers
    return side ? alloc_side(e) : FM_OK;
}

// ---- profiling helpers -----------------------------------------------------------
hipEvent_t get_ev(fm_engine* e)
{
    if (!e->ev_free.empty()) { hipEvent_t v = e->ev_free.back(); e->ev_free.pop_back(); return v; }
    hipEvent_t v = nullptr;
    if (hipEventCreate(&v) != hipSuccess) { e->prof_fail = true; return nullptr; }
    return v;
}
struct ProfScope {
    fm_engine* e; hipStream_t st; hipEvent_t a{}, b{}; int fam; double fl; bool on;
    ProfScope(fm_engine* e_, const Lane& L, int family, double flops) : e(e_), st(L.st), fam(family), fl(flops), on(e_->prof)
    {
        if (on) {
            a = get_ev(e); b = get_ev(e);
            on = a && b;
            if (on && hipEventRecord(a, st) != hipSuccess) { e->prof_fail = true; on = false; }
        }
    }
    ~ProfScope()
    {
        if (on) {
            if (hipEventRecord(b, st) != hipSuccess) e->prof_fail = true;
            e->evs.push_back({a, b, fam, fl});
        }
    }
};

struct OpScope {
    fm_engine* e; hipStream_t st; hipEvent_t a{}, b{}; int id = -1; bool on;
    OpScope(fm_engine* e_, const Lane& L, const char* op) : e(e_), st(L.st), on(e_->oprof)
    {
        lane_point(e_, &L == &e_->side);
        if (!on) return;
        char lab[96];
        snprintf(lab, sizeof lab, "%s@%d", op, e->ctx);
        for (size_t i = 0; i < e->op_names.size(); ++i)
            if (e->op_names[i] == lab) { id = (int)i; break; }
        if (id < 0) { id = (int)e->op_names.size(); e->op_names.push_back(lab); e->op_ms.push_back(0); e->op_n.push_back(0); }
        a = get_ev(e); b = get_ev(e);
        on = a && b && hipEventRecord(a, st) == hipSuccess;
    }
    ~OpScope()
    {
        if (on && hipEventRecord(b, st) == hipSuccess) e->opevs.push_back({a, b, id});
    }
};
#define OP(lane, name) OpScope os_(e, lane, name)
// a delay point without a profiling scope: ResNet-18's forwards, whose launches fm_profile_ops does not list
#define LP(lane) lane_point(e, &(lane) == &e->side)

// ---- layer launchers --------------------------------------------------------------
// operand prologue of a pointwise conv: Xe = swish(X*psc+psh)*gate, psc == null: X*gate, gate == null: none
struct Prologue { const float *psc = nullptr, *psh = nullptr, *gate = nullptr; };
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SWISH = 2 };      // the `act` of the kernels' epilogues
// epilogue of a forward conv: y = act(conv * scale + shift + res); scale == null: the raw output
struct Epilogue { const float *scale = nullptr, *shift = nullptr; In res; int act = ACT_NONE; };
// what a forward conv takes beyond operand and output; `stats`: where the BatchNorm partial sums of the raw output go
struct FwdOps { float* stats = nullptr; Prologue pro; Epilogue epi; };

// planes of an fp32 NHWC operand nobody produced planes for (test hooks): [C/32][3][npix][32] in the scratch buffer
const unsigned short* scratch_planes(fm_engine* e, Lane& L, const float* x, long long npix, int C)
{
    if ((size_t)npix * C * 3 > e->xp_scratch_elems) { soft(e, hipErrorInvalidValue); return nullptr; }
    // FM_DEBUG_REUSE_PLANES=1 (tools/probe_conv.py): time the GEMM alone -- the planes of the same operand are made once
    static const bool reuse = getenv("FM_DEBUG_REUSE_PLANES") && atoi(getenv("FM_DEBUG_REUSE_PLANES")) != 0;
    if (reuse && e->xp_scratch_src == x && e->xp_scratch_npix == npix) return e->xp_scratch;
    k_split_planes(x, e->xp_scratch, npix, C, L.st);
    e->xp_scratch_src = x; e->xp_scratch_npix = npix;
    return e->xp_scratch;
}
bool conv_uses_pconv(const fm_engine* e, const Conv& c, int imgs)
{
    return e->planes && c.pl_off >= 0 && pconv_takes(c.cout_p, c.cin_p, (long long)imgs * c.hin * c.win, c.win);
}

// the GEMM geometry of a convolution's forward / data-gradient launches -- taps, operand map, output grid: what pconv_uses_ts
// decides on and what launch_pconv and launch_igemm are handed.  The stem (cin == 3) has no tap list: its kernels walk kernel rows.
static void conv_fwd_geometry(const Conv& c, IgemmParams& p)
{
    p.ntaps = c.cin == 3 ? 0 : c.k * c.k;
    for (int t = 0; t < p.ntaps; ++t) { p.dh[t] = t / c.k - c.pad; p.dw[t] = t % c.k - c.pad; }
    p.M = c.cout_p;
    p.Hi = c.hin; p.Wi = c.win; p.Ci = c.cin_p;
    p.Hg = c.hout; p.Wg = c.wout; p.sg = c.stride;
}
static void conv_dgrad_geometry(const Conv& c, const DgradClass& d, IgemmParams& p)
{
    p.ntaps = d.taps.n;
    for (int t = 0; t < d.taps.n; ++t) { p.dh[t] = d.dh[t]; p.dw[t] = d.dw[t]; }
    p.M = c.cin_p;
    p.Hi = c.hout; p.Wi = c.wout; p.Ci = c.cout_p;
    p.Hg = (c.hin - d.ph + c.stride - 1) / c.stride;
    p.Wg = (c.win - d.pw + c.stride - 1) / c.stride;
    p.sg = 1;
}
static bool dgrad_uses_pconv(const fm_engine* e, const Conv& c, int imgs)
{
    return e->planes && c.ncls > 0 && c.cls[0].pl_off >= 0 && pconv_takes(c.cin_p, c.cout_p, (long long)imgs * c.hout * c.wout, c.wout);
}
// the operand shapes of the planes weight gradient: what pwgrad_takes admitted and pwgrad_ring_takes decides on
static bool wgrad_uses_pwgrad(const fm_engine* e, const Conv& c, int imgs)
{
    return e->planes && c.cin != 3 &&
           pwgrad_takes(c.cout_p, c.cin_p, c.k, (long long)imgs * c.hout * c.wout, (long long)imgs * c.hin * c.win, c.win, c.pad);
}
static void pwgrad_geometry(const fm_engine* e, const Conv& c, int imgs, PwgradParams& q)
{
    q.npix = (long long)imgs * c.hout * c.wout; q.xpix = (long long)imgs * c.hin * c.win;
    q.M = c.cout_p; q.Nw = c.Kw;
    q.Ho = c.hout; q.Wo = c.wout; q.Hi = c.hin; q.Wi = c.win; q.Ci = c.cin_p; q.stride = c.stride; q.pad = c.pad; q.ksz = c.k;
    q.sp = e->products;
}
// the shape fields of the fp32-operand weight gradient (wgrad.hip); the gather form of EfficientNet-B0's stem for the skinny kernels
static void wgrad_geometry(const fm_engine* e, const Conv& c, int imgs, WgradParams& p)
{
    p.sp = e->products;
    p.M = c.cout_p; p.Nw = c.Kw;
    p.Ho = c.hout; p.Wo = c.wout; p.Hi = c.hin; p.Wi = c.win; p.Ci = c.cin_p; p.stride = c.stride;
    if (c.stem3) { p.Hi = c.Hp; p.Wi = c.Wp; }      // gather table of build_tables: framed rows, no bounds
    p.npix = imgs * c.hout * c.wout;
    if (e->model == 1 && c.cin == 3) { p.gather_k = c.k; p.gather_pad = c.pad; p.gather_kw_p = c.kw_p; }
}

// The launcher conv_fwd / conv_dgrad / conv_wgrad hand conv c to for `imgs` images: the one decision they switch on, stats_tiles_for
// sizes the statistics by, the measurement family follows and fm_debug_conv_arm reports.  None: planes mode keeps no fp32 operands
// for the non-stem convs (activations exist only as planes, no row-major weight planes): a shape the planes kernel does not take is
// a graph error, not a reason to run the fp32-operand kernel on unwritten buffers.
enum class Arm { None, StemRows, PconvTs, PconvTap, PwConv, Igemm, IgemmStem, Pwgrad, PwgradRing, PwWgrad, WgradSkinny, WgradGeneric,
                 WgradGenericStem };

static Arm pconv_arm(const IgemmParams& geometry) { return pconv_uses_ts(geometry) ? Arm::PconvTs : Arm::PconvTap; }
static Arm fwd_arm(const fm_engine* e, const Conv& c, int imgs)
{
    if (e->stem_rows && c.stem3) return Arm::StemRows;
    if (conv_uses_pconv(e, c, imgs)) {
        IgemmParams p{};
        conv_fwd_geometry(c, p);
        return pconv_arm(p);
    }
    if (e->planes && c.cin != 3) return Arm::None;
    if (e->precision && (c.k == 1 || c.cin == 3)) return Arm::PwConv;      // bf16 storage + bf16 MFMA (pwconv_bf16.hip)
    return c.cin == 3 ? Arm::IgemmStem : Arm::Igemm;
}
// one launch per parity class: PconvTap if any class runs per tap (conv_dgrad asks pconv_arm about each class's own launch)
static Arm dgrad_arm(const fm_engine* e, const Conv& c, int imgs)
{
    if (dgrad_uses_pconv(e, c, imgs)) {
        for (int k = 0; k < c.ncls; ++k) {
            IgemmParams p{};
            conv_dgrad_geometry(c, c.cls[k], p);
            if (pconv_arm(p) == Arm::PconvTap) return Arm::PconvTap;
        }
        return Arm::PconvTs;
    }
    if (e->planes && c.cin != 3) return Arm::None;
    if (e->precision && c.k == 1) return Arm::PwConv;      // dX = dY W: the same streaming kernel with the transposed bf16 shadow
    return Arm::Igemm;
}
// launch_wgrad_skinny refuses exactly what wgrad_skinny_takes refuses (the slab only bounds its splits), so the skinny kernels are
// an arm of their own and nothing falls through to the generic kernel
static Arm wgrad_arm(const fm_engine* e, const Conv& c, int imgs)
{
    if (wgrad_uses_pwgrad(e, c, imgs)) {
        PwgradParams q{};
        pwgrad_geometry(e, c, imgs, q);
        return pwgrad_ring_takes(q) ? Arm::PwgradRing : Arm::Pwgrad;
    }
    if (e->planes && c.cin != 3) return Arm::None;
    if (e->precision && (c.k == 1 || c.cin == 3)) return Arm::PwWgrad;
    if (e->model == 1 && (c.k == 1 || c.cin == 3)) {
        WgradParams p{};
        wgrad_geometry(e, c, imgs, p);
        if (wgrad_skinny_takes(p)) return Arm::WgradSkinny;
    }
    return c.cin == 3 ? Arm::WgradGenericStem : Arm::WgradGeneric;
}
// measurement families follow the kernel symbols: M = the rows of the GEMM (>= 128: the 128-row tiles).  0 / 1 = igemm and
// pconv_kernel<4 | 2, ..., true> (tap rows shared), 6 / 7 = <..., false>, 2 = the stem kernels, 3 / 4 / 5 / 8 = the weight gradients
static int prof_family(Arm a, int M)
{
    const bool big = M >= 128;
    switch (a) {
    case Arm::StemRows: case Arm::IgemmStem: return 2;
    case Arm::PconvTs: case Arm::Igemm: return big ? 0 : 1;
    case Arm::PconvTap: return big ? 6 : 7;
    case Arm::Pwgrad: case Arm::WgradGeneric: return big ? 3 : 4;
    case Arm::WgradGenericStem: return big ? 3 : 5;
    case Arm::WgradSkinny: return 4;
    case Arm::PwgradRing: return 8;
    default: return -1;      // the bf16 pointwise launchers are not measured by family
    }
}

// partial-sum tiles per group the forward GEMM of conv c leaves in `stats`, one per pixel tile of its grid (pro_gate: this call
// carries an operand prologue)
static int stats_tiles_for(Arm fwd, const Conv& c, int imgs_per_group, int groups, bool pro_gate)
{
    const int pix = imgs_per_group * c.hout * c.wout;
    auto tiles = [&](int bn) { return (pix + bn - 1) / bn; };
    switch (fwd) {
    case Arm::StemRows: return stem_rows_stats_tiles(imgs_per_group, c.hout);
    case Arm::PwConv: return pw_blocks(pix, groups, c.cout_p, c.cin == 3 ? c.Kw : c.cin_p, pro_gate, c.hout * c.wout);
    case Arm::PconvTs: case Arm::PconvTap: return tiles(pconv_tile_n(c.cout_p));
    default: return tiles(igemm_tile_n(c.cout_p, c.cin == 3));
    }
}

// The forward conv in its raw form (no FwdOps: the test hooks) and as conv_fwd_train / conv_fwd_eval hand it on.  The planes
// kernels read x.p, write y.p and add res.p; only their eval epilogue writes planes, and y.f may then be null
void conv_fwd(fm_engine* e, Lane& L, int ci, const Weights& W, In x, Out y, int imgs, int groups, const FwdOps& o = {})
{
    Conv& c = e->convs[ci];
    const Epilogue& ep = o.epi;
    const Prologue& pro = o.pro;
    float* const stats = o.stats;
    const Arm arm = fwd_arm(e, c, imgs);
    const int tiles_n = stats_tiles_for(arm, c, imgs / groups, groups, pro.gate != nullptr);
    if (stats) { e->stats_conv = ci; e->stats_tiles_n = tiles_n; }
    const int fam = prof_family(arm, c.cout_p);
    const double flops = 2.0 * c.macs_per_img * imgs;
    switch (arm) {
    case Arm::StemRows: {                    // `x` is ignored: the operand is the framed image's planes (to_nhwc4)
        StemRowsParams q{};
        q.Xp = e->x3p + (size_t)e->in_img0 * c.Hp * c.Wp * 4; q.Wst = W.wst; q.Y = y.f;
        q.scale = ep.scale; q.shift = ep.shift; q.stats = stats; q.relu = ep.act;
        q.imgs = imgs; q.imgs_per_group = imgs / groups; q.Hp = c.Hp; q.Wp = c.Wp; q.Ho = c.hout; q.Wo = c.wout;
        q.sp = e->products; q.plane_bytes = e->x3p_plane_elems * 2;
        ProfScope ps(e, L, fam, flops);
        launch_stem_rows(q, L.st);
        return;
    }
    case Arm::PwConv: {
        const bool stem16 = c.cin == 3;      // `x` is ignored: the operand is the im2col matrix
        PwParams q{};
        q.zeros = e->zeros;
        q.W = W.wb + c.wb_off;
        q.X = reinterpret_cast<const bf16*>(stem16 ? e->stem_col : x.f); q.Y = reinterpret_cast<bf16*>(y.f);
        if (stem16) q.X += (size_t)e->in_img0 * c.hout * c.wout * c.Kw;
        q.M = c.cout_p; q.K = stem16 ? c.Kw : c.cin_p;
        q.npix = (imgs / groups) * c.hout * c.wout; q.groups = groups;
        q.scale = ep.scale; q.shift = ep.shift; q.res = reinterpret_cast<const bf16*>(ep.res.f); q.act = ep.act;
        q.stats = stats;
        if (pro.gate) { q.psc = pro.psc; q.psh = pro.psh; q.gate = pro.gate; }
        q.HW = c.hout * c.wout;
        launch_pw_conv(q, L.st);
        return;
    }
    case Arm::PconvTs: case Arm::PconvTap: case Arm::Igemm: case Arm::IgemmStem: break;      // one parameter block, below
    default: soft(e, hipErrorInvalidValue); return;
    }
    IgemmParams p{};
    p.Y = y.f; p.slab = L.sk_slab; p.counters = L.sk_counters; p.err = e->dev_err; p.err_host = e->host_err_dev; p.sp = e->products;
    conv_fwd_geometry(c, p);
    p.res = ep.res.f; p.scale = ep.scale; p.shift = ep.shift; p.stats = stats;
    p.Ho = c.hout; p.Wo = c.wout; p.Co = c.cout_p;
    p.os = 1; p.oh0 = 0; p.ow0 = 0;
    p.imgs_per_group = imgs / groups;
    p.tilesN = tiles_n;
    p.relu = ep.act;
    if (arm == Arm::PconvTs || arm == Arm::PconvTap) {
        p.xp_pix = (long long)imgs * c.hin * c.win;
        p.Xp = x.p ? x.p : scratch_planes(e, L, x.f, p.xp_pix, c.cin_p);
        p.Wsp = W.wpl_f + c.pl_off;
        p.Yp = y.p; p.yp_pix = (long long)imgs * c.hout * c.wout; p.resp = ep.res.p;
        p.tilesM = c.cout_p / pconv_tile_m(c.cout_p);
        ProfScope ps(e, L, fam, flops);
        launch_pconv(p, groups, L.st);
        return;
    }
    p.W = W.state + c.w_off; p.X = x.f; p.zeros = e->zeros; p.nsteps = c.nsteps;
    if (!e->planes && c.pl_off >= 0) p.Wsp = W.wpl_f + c.pl_off;      // row-major planes
    if (c.cin == 3) {
        p.stem_kw = c.k; p.stem_pad = c.pad; p.stem_h2 = c.kw_p == 8 ? 1 : 0; p.stem3 = c.stem3 ? 1 : 0;
        if (c.stem3) p.X = e->x3 + (size_t)e->in_img0 * c.Hp * c.Wp * 3;     // `x` is ignored: the operand is the framed NHWC3 image
        else p.X = x.f + (size_t)e->in_img0 * c.hin * c.win * 4;
    }
    if (c.stem3) { p.Hi = c.Hp; p.Wi = c.Wp; }
    if (pro.gate) {       // fp32 project conv: only the streaming kernel (conv1x1.hip) applies the gate (eval) or BN1 + Swish + gate (train)
        p.gate = pro.gate; p.gate_HW = c.hout * c.wout; p.psc = pro.psc; p.psh = pro.psh;
        // the streaming kernel has a gate-only eval form (no statistics) and a BN1 + Swish + gate train form (statistics): a
        // gate-only prologue WITH statistics, or a full prologue without them, has no instantiation
        if (!conv1x1_stream_takes(c.cin_p, c.cout_p, c.cout_p) || c.k != 1 || c.stride != 1 || (pro.psc && !stats) ||
            (!pro.psc && stats))
            soft(e, hipErrorInvalidValue);
    }
    p.tilesM = (c.cout_p + igemm_tile_m(c.cout_p) - 1) / igemm_tile_m(c.cout_p);
    ProfScope ps(e, L, fam, flops);
    launch_igemm(p, groups, L.st);
}

// tiles per group of the partial sums conv ci's forward left in ws_stats (set by that conv_fwd call; asking for another conv's
// is a graph error: the buffer holds one conv's partials at a time)
int stats_tiles(fm_engine* e, int ci)
{
    if (e->stats_conv != ci) soft(e, hipErrorInvalidValue);
    return e->stats_tiles_n;
}

// what a data gradient adds to its output: a residual, or (stride-2 convs) dx's own contents at parity class (0,0)
struct DgradAdd { const float* res = nullptr; bool acc_cls0 = false; };
// dx[imgs][hin][win][cin] = dgrad(dy[imgs][hout][wout][cout])
void conv_dgrad(fm_engine* e, Lane& L, int ci, In dy, float* dx, int imgs, const DgradAdd& add = {})
{
    Conv& c = e->convs[ci];
    const Arm arm = dgrad_arm(e, c, imgs);
    const long long xp_pix = (long long)imgs * c.hout * c.wout;
    switch (arm) {
    case Arm::PwConv: {
        PwParams q{};
        q.zeros = e->zeros;
        q.W = e->student.wb + c.wbt_off;
        q.X = reinterpret_cast<const bf16*>(dy.f); q.Y = reinterpret_cast<bf16*>(dx);
        q.M = c.cin_p; q.K = c.cout_p;
        q.npix = imgs * c.hout * c.wout; q.groups = 1;
        q.res = reinterpret_cast<const bf16*>(add.res);
        q.HW = c.hout * c.wout;
        launch_pw_conv(q, L.st);
        return;
    }
    case Arm::PconvTs: case Arm::PconvTap: case Arm::Igemm: break;      // one launch per parity class, below
    default: soft(e, hipErrorInvalidValue); return;
    }
    const bool planes = arm != Arm::Igemm;
    if (planes && !dy.p) dy.p = scratch_planes(e, L, dy.f, xp_pix, c.cout_p);
    for (int k = 0; k < c.ncls; ++k) {
        DgradClass& d = c.cls[k];
        IgemmParams p{};
        p.Y = dx; p.slab = L.sk_slab; p.counters = L.sk_counters; p.err = e->dev_err; p.err_host = e->host_err_dev; p.sp = e->products;
        conv_dgrad_geometry(c, d, p);
        p.res = add.res ? add.res : ((add.acc_cls0 && d.ph == 0 && d.pw == 0) ? dx : nullptr);
        p.Ho = c.hin; p.Wo = c.win; p.Co = c.cin_p;
        p.os = c.stride; p.oh0 = d.ph; p.ow0 = d.pw;
        p.imgs_per_group = imgs;
        p.relu = 0;
        const int bn = planes ? pconv_tile_n(c.cin_p) : igemm_tile_n(c.cin_p);
        p.tilesN = (imgs * p.Hg * p.Wg + bn - 1) / bn;
        const double flops = 2.0 * c.macs_per_img * imgs * d.taps.n / (double)(c.k * c.k);
        if (planes) {
            p.Xp = dy.p; p.xp_pix = xp_pix; p.Wsp = e->wpl_d + d.pl_off;
            p.tilesM = c.cin_p / pconv_tile_m(c.cin_p);
            ProfScope ps(e, L, prof_family(pconv_arm(p), c.cin_p), flops);       // this class's own kernel
            launch_pconv(p, 1, L.st);
        } else {
            p.W = d.wpack; p.X = dy.f; p.zeros = e->zeros; p.nsteps = d.nsteps;
            if (!e->planes && d.pl_off >= 0) p.Wsp = e->wpl_d + d.pl_off;
            p.tilesM = (c.cin_p + igemm_tile_m(c.cin_p) - 1) / igemm_tile_m(c.cin_p);
            ProfScope ps(e, L, prof_family(arm, c.cin_p), flops);
            launch_igemm(p, 1, L.st);
        }
    }
}

// The input gradient of a stride-2 residual block, dx = dgrad(c1; dy1) + dgrad(ds; dyd), as ONE launch of the per-tap planes kernel
// (pconv.hip job table): one job per parity class of the 3x3 conv; the 1x1 downsample's only class, (0,0), has the tap of the
// 3x3's class (0,0) -- the same dy pixel -- and the same output grid: its K-steps ride behind that job's own, with dyd's planes
// as the job's second operand.  Every element of dx is written once; nothing is read back.  false = the shapes are not of that
// kind (or not planes mode): the caller runs the two conv_dgrad calls.
bool block_dgrad(fm_engine* e, Lane& L, int c1i, int dsi, In dy1, In dyd, float* dx, int imgs)
{
    Conv& c = e->convs[c1i];
    Conv& d = e->convs[dsi];
    const long long xp_pix = (long long)imgs * c.hout * c.wout;
    if (c.ncls != 4 || d.ncls != 1 || !dgrad_uses_pconv(e, c, imgs) || d.cls[0].pl_off < 0) return false;
    static_assert(PCONV_MAX_JOBS >= 4, "one job per parity class");
    const DgradClass& d0 = d.cls[0];
    if (c.stride != 2 || d.stride != 2 || d.k != 1 || d.cin_p != c.cin_p || d.cout_p != c.cout_p || d.hin != c.hin || d.win != c.win ||
        d.hout != c.hout || d.wout != c.wout || d0.ph != 0 || d0.pw != 0 || d0.dh[0] != 0 || d0.dw[0] != 0)
        return false;
    const DgradClass& c0 = c.cls[0];
    if (c0.ph != 0 || c0.pw != 0 || c0.taps.n != 1 || c0.dh[0] != 0 || c0.dw[0] != 0) return false;
    if (!dy1.p) dy1.p = scratch_planes(e, L, dy1.f, xp_pix, c.cout_p);
    if (!dyd.p) {
        if ((size_t)xp_pix * d.cout_p * 3 > e->xp_scratch_elems) { soft(e, hipErrorInvalidValue); return true; }
        k_split_planes(dyd.f, e->xp_scratch2, xp_pix, d.cout_p, L.st);
        dyd.p = e->xp_scratch2;
    }
    if (!dy1.p) return true;                    // (scratch_planes reported it)
    IgemmParams p{};
    p.Xp = dy1.p; p.Xp2 = dyd.p; p.xp_pix = xp_pix; p.Wsp = e->wpl_d;
    p.Y = dx; p.slab = L.sk_slab; p.counters = L.sk_counters; p.err = e->dev_err; p.err_host = e->host_err_dev; p.sp = e->products;
    p.M = c.cin_p;
    p.Hi = c.hout; p.Wi = c.wout; p.Ci = c.cout_p;
    p.sg = 1;
    p.Ho = c.hin; p.Wo = c.win; p.Co = c.cin_p;
    p.os = c.stride;
    p.imgs_per_group = imgs;
    p.tilesM = c.cin_p / pconv_tile_m(c.cin_p);
    p.relu = 0;
    p.njobs = c.ncls;
    for (int k = 0; k < c.ncls; ++k) {
        const DgradClass& q = c.cls[k];
        PconvJob& j = p.job[k];
        j.ntaps = q.taps.n; j.tapcode = pconv_tapcode(q.dh, q.dw, q.taps.n);
        j.cib = j.icc2 = c.cout_p >> 5;
        j.wofs = j.wofs2 = (unsigned)(q.pl_off * 2);
        j.Hg = (c.hin - q.ph + c.stride - 1) / c.stride;
        j.Wg = (c.win - q.pw + c.stride - 1) / c.stride;
        j.oh0 = q.ph; j.ow0 = q.pw;
    }
    p.job[0].cib += d.cout_p >> 5;
    p.job[0].wofs2 = (unsigned)(d0.pl_off * 2);
    // the per-tap kernel's family; the launch's algorithmic FLOPs = both convs'
    ProfScope ps(e, L, prof_family(Arm::PconvTap, c.cin_p), 2.0 * (c.macs_per_img + d.macs_per_img) * imgs);
    launch_pconv(p, 1, L.st);
    return true;
}

// pro: the operand x is re-formed on load (bf16 project conv), its BatchNorm statistics per group of pix_per_group pixels
void conv_wgrad(fm_engine* e, Lane& L, int ci, In x, In dy, int imgs, const Prologue& pro = {}, int pix_per_group = 0)
{
    const Conv& c = e->convs[ci];
    const Arm arm = wgrad_arm(e, c, imgs);
    const int fam = prof_family(arm, c.cout_p);
    const double flops = 2.0 * c.macs_per_img * imgs;
    int sk = 0;                              // partial slabs the arm's kernel leaves in L.ws_slab
    switch (arm) {
    case Arm::Pwgrad:
    case Arm::PwgradRing: {
        PwgradParams q{};
        pwgrad_geometry(e, c, imgs, q);
        if (!x.p) x.p = scratch_planes(e, L, x.f, q.xpix, c.cin_p);
        if (!dy.p) {
            if ((size_t)q.npix * c.cout_p * 3 > e->xp_scratch_elems) { soft(e, hipErrorInvalidValue); return; }
            k_split_planes(dy.f, e->xp_scratch2, q.npix, c.cout_p, L.st);
            dy.p = e->xp_scratch2;
        }
        q.dYp = dy.p; q.Xp = x.p; q.slab = L.ws_slab;
        ProfScope ps(e, L, fam, flops);
        sk = arm == Arm::PwgradRing ? launch_pwgrad_ring(q, e->slab_floats, L.st) : launch_pwgrad(q, e->slab_floats, L.st);
        if (sk <= 0) soft(e, hipErrorInvalidValue);
        break;
    }
    case Arm::PwWgrad: {
        const bool stem16 = c.cin == 3;
        PwWgradParams q{};
        q.dY = reinterpret_cast<const bf16*>(dy.f); q.X = reinterpret_cast<const bf16*>(stem16 ? e->stem_col : x.f);
        q.slab = L.ws_slab; q.M = c.cout_p; q.K = stem16 ? c.Kw : c.cin_p; q.npix = imgs * c.hout * c.wout;
        if (pro.gate) { q.psc = pro.psc; q.psh = pro.psh; q.gate = pro.gate; }
        q.HW = c.hout * c.wout; q.pix_per_group = pix_per_group ? pix_per_group : q.npix;
        sk = launch_pw_wgrad(q, e->slab_floats, L.st);
        if (sk <= 0) g_err = "pw_wgrad: shape not handled";
        break;
    }
    case Arm::WgradSkinny:
    case Arm::WgradGeneric:
    case Arm::WgradGenericStem: {
        WgradParams p{};
        p.dY = dy.f; p.X = x.f; p.slab = L.ws_slab; p.tab = c.tab; p.zeros = e->zeros;
        wgrad_geometry(e, c, imgs, p);
        if (c.stem3) p.X = e->x3;
        ProfScope ps(e, L, fam, flops);
        if (arm == Arm::WgradSkinny) {
            sk = launch_wgrad_skinny(p, e->slab_floats, L.st);
            if (sk <= 0) soft(e, hipErrorInvalidValue);
            break;
        }
        const int bm = c.cout_p >= 128 ? 128 : 64, bn = wgrad_tile_n(c.cout_p, c.Kw);
        p.bn = bn;
        p.tilesM = (c.cout_p + bm - 1) / bm;
        p.tilesN = (c.Kw + bn - 1) / bn;
        const int tiles = p.tilesM * p.tilesN;
        // tiles * splits <= 512 = ONE round of the 512 block slots: with the weight gradients on the side stream next to the
        // BN-backward / data-gradient chain, a second round of their blocks holds slots the main stream's next GEMM is waiting for
        // (two-stream step 36.8 -> 36.3 ms; one stream: 38.5 either way; 384: 37.3, 640: 37.4, 1024 = round 2's choice)
        constexpr int WG_SLOTS = 512;
        int splits = std::max(1, WG_SLOTS / tiles);
        const int max_by_pix = std::max(1, p.npix / 256);
        const int max_by_mem = (int)std::max<size_t>(1, e->slab_floats / c.w_numel);
        splits = std::max(1, std::min(splits, std::min(max_by_pix, max_by_mem)));
        p.pix_per_split = (((p.npix + splits - 1) / splits) + 31) & ~31;
        sk = (p.npix + p.pix_per_split - 1) / p.pix_per_split;
        if (!launch_wgrad(p, sk, L.st)) soft(e, hipErrorInvalidValue);     // surfaces through STEP_DONE as FM_ERR_HIP
        break;
    }
    default: soft(e, hipErrorInvalidValue); return;
    }
    if (sk > 0) k_reduce_slabs(L.ws_slab, e->grad + c.w_off, sk, (int64_t)c.w_numel, L.st);
    if (c.stem3) k_stem3_mask_grad(e->grad + c.w_off, c.cout_p, L.st);
}

// where BatchNorm b's parameters live: the student's gamma / beta / running statistics and the gradient arena's dgamma / dbeta
struct BnSlots { float *gamma, *beta, *run_mean, *run_var, *dgamma, *dbeta; };
BnSlots bn_slots(const fm_engine* e, const Bn& b)
{
    float *S = e->student.state + b.ch_off, *G = e->grad + b.ch_off;
    return {S + e->off_gamma, S + e->off_beta, S + e->off_rm, S + e->off_rv, G + e->off_gamma, G + e->off_beta};
}

// frozen statistics: mean / istd / scale / shift of every group from the running statistics, which stay as they are
void bn_fwd_fixed(fm_engine* e, Lane& L, Bn& b, int groups)
{
    const BnSlots s = bn_slots(e, b);
    k_bn_finalize_frozen(groups, b.C, s.gamma, s.beta, s.run_mean, s.run_var, b.mean, b.istd, b.scale, b.shift, e->bn_eps, L.st, e->dev_err);
}
// The finalize of a train-mode BatchNorm bi from `tiles` partial sums per group in `part`, `count` values per group and channel;
// the running statistics and the counter move in BnMode::Batch alone.  skip: the step's skip word, where the caller has one
void bn_fwd_stats(fm_engine* e, Lane& L, int bi, const float* part, int groups, int tiles, int count, BnMode mode, const int* skip)
{
    Bn& b = e->bns[bi];
    if (mode == BnMode::Frozen) { bn_fwd_fixed(e, L, b, groups); return; }
    const BnSlots s = bn_slots(e, b);
    const bool run = mode == BnMode::Batch;
    k_bn_finalize(part, groups, tiles, b.C, count, s.gamma, s.beta, run ? s.run_mean : nullptr, run ? s.run_var : nullptr, b.mean, b.istd,
                  b.scale, b.shift, e->bn_eps, e->bn_mom, L.st, skip);
    if (run) e->student.counters[bi] += groups;
}
// BN statistics of conv `ci`'s output (partials left in ws_stats by the conv epilogue)
void bn_fwd_finalize(fm_engine* e, Lane& L, int ci, int groups, int imgs_per_group, BnMode mode)
{
    const Conv& c = e->convs[ci];
    // (frozen statistics read no partials: nothing is asked of ws_stats)
    const int tiles = mode == BnMode::Frozen ? 0 : stats_tiles(e, ci);
    bn_fwd_stats(e, L, c.bn, e->ws_stats, groups, tiles, imgs_per_group * c.hout * c.wout, mode, e->dev_err);
}

// The forward conv as the train graphs run it: the raw output into Conv::y, its partial statistics into ws_stats, then the
// BatchNorm finalize.  op: the conv's label for fm_profile_ops (EfficientNet-B0); ResNet-18's forwards are delay points only
void conv_fwd_train(fm_engine* e, Lane& L, int ci, const Weights& W, In x, int groups, int B, BnMode mode, const char* op = nullptr,
                    const Prologue& pro = {})
{
    const Out y{e->convs[ci].y};
    const FwdOps o{.stats = e->ws_stats, .pro = pro};
    if (op) {
        { OP(L, op); conv_fwd(e, L, ci, W, x, y, groups * B, groups, o); }
        { OP(L, "bn_fwd_finalize"); bn_fwd_finalize(e, L, ci, groups, B, mode); }
    } else {
        LP(L); conv_fwd(e, L, ci, W, x, y, groups * B, groups, o);
        LP(L); bn_fwd_finalize(e, L, ci, groups, B, mode);
    }
}
// ... and as the eval graphs do: BatchNorm folded into the epilogue (W's eval affine of the conv's BatchNorm), one group
void conv_fwd_eval(fm_engine* e, Lane& L, int ci, const Weights& W, In x, Out y, int imgs, int act, In res = {}, const Prologue& pro = {})
{
    const int ch = e->bns[e->convs[ci].bn].ch_off;
    conv_fwd(e, L, ci, W, x, y, imgs, 1, {.pro = pro, .epi = {W.ev_scale + ch, W.ev_shift + ch, res, act}});
}

// The finalize of BatchNorm b's backward from `partials` partial sums per group in ws_part: the coefficients ca / cb / cc of the
// apply pass, dgamma and dbeta
void bn_bwd_finalize(fm_engine* e, Lane& L, const Bn& b, int groups, int partials, int count, bool frozen)
{
    const BnSlots s = bn_slots(e, b);
    k_bn_bwd_finalize(e->ws_part, groups, partials, b.C, count, s.gamma, b.mean, b.istd, e->ca, e->cb, e->cc, s.dgamma, s.dbeta, L.st, frozen);
}
// Where bn_bwd takes the mask of the ReLU behind the BatchNorm from.  Z: the fp32 z; ZPlane: z is kept only as planes, the mask is
// the sign of its h plane; OwnOutput: z = relu(bn(y)) of THIS BatchNorm with nothing added (bn1 of a basic block): the mask is
// recomputed from y, which both passes read anyway, and z is not read (FM_BN_MASK_FROM_Y=0 reads an fp32 z as before)
enum class Mask { None, Z, ZPlane, OwnOutput };
// backward through BN bi: dz -> dy in the forms dy names (planes: what the data gradient reads); dyh_out: the masked gradient
void bn_bwd(fm_engine* e, Lane& L, int bi, const float* dz, Out dy, int groups, int imgs_per_group, bool frozen, Mask mask = Mask::None,
            In z = {}, float* dyh_out = nullptr)
{
    const Conv& c = e->convs[bi];
    Bn& b = e->bns[bi];
    const int pix = imgs_per_group * c.hout * c.wout;
    const char* fy = getenv("FM_BN_MASK_FROM_Y");          // read per call: tests compare both forms in one process
    const int from_y = fy ? atoi(fy) : 1;
    const float *msc = nullptr, *msh = nullptr, *zf = nullptr;
    const unsigned short* zh = nullptr;
    if (mask == Mask::Z || (mask == Mask::OwnOutput && !from_y && z.f)) zf = z.f;
    else if (mask == Mask::ZPlane) zh = z.p;
    else if (mask == Mask::OwnOutput) { msc = b.scale; msh = b.shift; }
    k_bn_bwd_reduce(dz, zf, c.y, b.mean, b.istd, e->ws_part, groups, pix, b.C, L.st, msc, msh, zh);
    bn_bwd_finalize(e, L, b, groups, bn_bwd_blocks(pix), pix, frozen);
    if (dy.p) k_bn_bwd_apply_planes(dz, zf, c.y, e->ca, e->cb, e->cc, dy.f, dy.p, dyh_out, groups, pix, b.C, L.st, msc, msh, zh);
    else k_bn_bwd_apply(dz, zf, c.y, e->ca, e->cb, e->cc, dy.f, dyh_out, groups, pix, b.C, L.st, msc, msh);
}

void to_nhwc4(fm_engine* e, Lane& L, const float* const* xs, int groups, int B)
{
    if (e->precision && e->model == 1) {      // bf16 EfficientNet: the stem reads an im2col matrix (teacher, student and wgrad share it)
        const Conv& c = e->convs[e->c_stem];
        for (int g = 0; g < groups; ++g)
            k_stem_im2col(xs[g], reinterpret_cast<bf16*>(e->stem_col) + (size_t)g * B * c.hout * c.wout * c.Kw, B, e->H, e->W, c.hout,
                          c.wout, c.k, c.stride, c.pad, c.pad, L.st);
        return;
    }
    if (e->convs[0].stem3) {
        const Conv& c = e->convs[0];
        for (int g = 0; g < groups; ++g)
            k_frame_nhwc3(xs[g], e->x3 + (size_t)g * B * c.Hp * c.Wp * 3, B, e->H, e->W, c.Hp, c.Wp, 3, 3, 0, L.st,
                          e->stem_rows ? e->x3p + (size_t)g * B * c.Hp * c.Wp * 4 : nullptr, e->x3p_plane_elems);
        return;
    }
    for (int g = 0; g < groups; ++g)
        k_nchw_to_nhwc4(xs[g], e->x4 + (size_t)g * B * e->H * e->W * 4, B, e->H, e->W, L.st);
}

// ---- coherence of the copies derived from a net's state ----------------------------------------------------------
// The staleness flags are raised in the two functions below and nowhere else, and cleared only by the ensure_* function that
// remakes the copy (tests/test_coherence_cpu.py holds both).
// fm_teacher_swap alone calls this directly: the copies only the student has were made for the net that left its slot
void student_copies_stale(fm_engine* e)
{
    e->dgrad_dirty = true;
    e->stem_dpack_stale = true;
}
// Net W's state changed: its weights (and whatever else), or -- second form -- only its BatchNorm running statistics, which
// nothing but the folded eval affine reads.  Every entry point that writes a state, or hands out the pointer to it, says so here.
enum class Moved { Weights, Stats };
void net_changed(fm_engine* e, Weights& W, Moved what = Moved::Weights)
{
    W.ev_dirty = true;
    if (what == Moved::Stats) return;
    W.fwd_dirty = true;
    if (&W == &e->student) student_copies_stale(e);
}
// the folded eval BatchNorm affine of W, on the lane the forward that reads it runs on
void ensure_eval_affine(fm_engine* e, Lane& L, Weights& W)
{
    if (!W.ev_dirty) return;
    const float* S = W.state;
    k_bn_eval_affine(S + e->off_gamma, S + e->off_beta, S + e->off_rm, S + e->off_rv, W.ev_scale, W.ev_shift, e->n_bn_ch, e->bn_eps, L.st);
    W.ev_dirty = false;
}
// Everything else derived from the weights is (re)made on the main lane, where the weights change.
// W's forward shadows: the bf16 cast of the 1x1 convs, or the weight planes in the engine's layout and the stem's planes
void ensure_fwd_shadows(fm_engine* e, Weights& W)
{
    if (!W.fwd_dirty) return;
    Lane& L = e->main;
    if (e->precision) launch_cast_weights(W.state, W.wb, e->cast_jobs.jobs, e->cast_jobs.n, e->cast_jobs.blocks, L.st);
    else if (e->planes) {
        k_split_weights_bm(W.state, W.wpl_f, e->split_f.jobs, e->split_f.n, e->split_f.blocks, L.st);
        if (e->stem_rows) k_stem_weight_planes(W.state + e->convs[0].w_off, W.wst, e->convs[0].Kw, L.st);
    } else
        k_split_weights(W.state, W.wpl_f, e->split_f.jobs, e->split_f.n, e->split_f.blocks, L.st);
    W.fwd_dirty = false;
}
// the student's forward shadows and what only the student has: the transposed weight packs of every data-gradient GEMM, all in
// ONE launch, then the planes of the packs just made
void ensure_packed(fm_engine* e)
{
    ensure_fwd_shadows(e, e->student);
    if (!e->dgrad_dirty) return;
    Lane& L = e->main;
    if (!e->precision && e->pack_jobs.n)
        k_pack_dgrad_all(e->student.state, e->pack_jobs.jobs, e->pack_jobs.n, e->pack_jobs.blocks, L.st);
    (e->planes ? k_split_weights_bm : k_split_weights)(nullptr, e->wpl_d, e->split_d.jobs, e->split_d.n, e->split_d.blocks, L.st);
    e->dgrad_dirty = false;
}

// train-mode forward (the student's) of groups*B images already in e->x4; fills A and feat/logits
void forward_train(fm_engine* e, Lane& L, Acts& A, int groups, int B, BnMode mode)
{
    const int imgs = groups * B;
    const Weights& W = e->student;
    const float* S = W.state;
    Conv& c0 = e->convs[0];
    conv_fwd_train(e, L, 0, W, {e->x4}, groups, B, mode);
    LP(L);
    if (A.p0.p) k_stem_pool_planes(c0.y, e->bns[0].scale, e->bns[0].shift, A.p0.f, e->idx0, A.p0.p, groups, B, c0.hout, c0.wout, 64, L.st);
    else k_stem_pool(c0.y, e->bns[0].scale, e->bns[0].shift, A.p0.f, e->idx0, groups, B, c0.hout, c0.wout, 64, L.st);
    // BatchNorm apply of conv ci's output into `out`: + the residual `res`, or + BatchNorm ds of the downsample conv's output; ReLU.
    // Planes mode: the activations z1 / out exist ONLY as planes (what the conv GEMMs read; the residual add and the ReLU masks of
    // the backward re-form the fp32 value / its sign from them) -- except the last block's `out`, which feeds the average pool:
    // fp32 only
    auto apply = [&](int ci, Out out, In res = {}, int ds = -1) {
        const Conv& c = e->convs[ci];
        const Bn& b = e->bns[ci];
        const float* y2 = ds >= 0 ? e->convs[ds].y : nullptr;
        const float *s2 = y2 ? e->bns[ds].scale : nullptr, *h2 = y2 ? e->bns[ds].shift : nullptr;
        const int pix = B * c.hout * c.wout;
        LP(L);
        if (out.p) k_bn_apply_planes(c.y, b.scale, b.shift, res.f, y2, s2, h2, out.f, out.p, groups, pix, c.cout, 1, L.st, res.p);
        else k_bn_apply(c.y, b.scale, b.shift, res.f, y2, s2, h2, out.f, groups, pix, c.cout, 1, L.st);
    };
    In cur = A.p0;                       // the block's input in the forms that are valid (p0 is written both ways)
    for (size_t bi = 0; bi < e->blocks.size(); ++bi) {
        const Block& blk = e->blocks[bi];
        BlockActs& a = A.blk[bi];
        const Conv& c1 = e->convs[blk.c1];
        const bool last = bi + 1 == e->blocks.size();
        conv_fwd_train(e, L, blk.c1, W, cur, groups, B, mode);
        apply(blk.c1, kept(a.z1));
        conv_fwd_train(e, L, blk.c2, W, kept(a.z1), groups, B, mode);
        const Out out = last ? Out{a.out.f} : kept(a.out);
        if (blk.ds >= 0) {
            conv_fwd_train(e, L, blk.ds, W, cur, groups, B, mode);
            apply(blk.c2, out, {}, blk.ds);
        } else {
            In idt = cur.f ? In{cur.f} : cur;
            if (last && !idt.f) {      // the last block adds a planes-only residual into an fp32 output: re-form the residual first
                float* f32 = A.blk[bi - 1].out.f;
                LP(L); k_planes_to_f32(cur.p, f32, (long long)imgs * c1.hin * c1.win, c1.cin, L.st);
                idt = {f32};
            }
            apply(blk.c2, out, idt);
        }
        cur = out;
    }
    const Conv& cl = e->convs[e->blocks.back().c2];
    LP(L); k_avgpool(cur.f, DT_F32, e->feat, imgs, cl.hout * cl.wout, 512, L.st);
    LP(L); k_fc_fwd(e->feat, S + e->off_fcw, S + e->off_fcb, e->logits, imgs, 512, e->C, L.st);
    if (mode != BnMode::Frozen) net_changed(e, e->student, Moved::Stats);
}

// eval-mode forward (BN folded into the conv epilogue) of `imgs` images in e->x4
void forward_eval(fm_engine* e, Lane& L, Weights& W, Acts& A, int imgs, float* feat, float* logits)
{
    const float* S = W.state;
    LP(L); ensure_eval_affine(e, L, W);
    Conv& c0 = e->convs[0];
    LP(L); conv_fwd_eval(e, L, 0, W, {e->x4}, {A.stem_y}, imgs, ACT_RELU);
    LP(L);
    if (A.p0.p) k_stem_pool_planes(A.stem_y, nullptr, nullptr, A.p0.f, nullptr, A.p0.p, 1, imgs, c0.hout, c0.wout, 64, L.st);
    else k_stem_pool(A.stem_y, nullptr, nullptr, A.p0.f, nullptr, 1, imgs, c0.hout, c0.wout, 64, L.st);
    In cur = A.p0;
    for (size_t bi = 0; bi < e->blocks.size(); ++bi) {
        const Block& blk = e->blocks[bi];
        BlockActs& a = A.blk[bi];
        // planes mode: z1 and `out` exist only as planes (the next convs read them; the next block's residual add re-forms the fp32
        // values in the epilogue) -- except the last block's `out`, which feeds the average pool: fp32 only
        const bool last = bi + 1 == e->blocks.size();
        LP(L); conv_fwd_eval(e, L, blk.c1, W, cur, kept(a.z1), imgs, ACT_RELU);
        In idt = cur.f ? In{cur.f} : cur;
        if (blk.ds >= 0) {
            LP(L); conv_fwd_eval(e, L, blk.ds, W, cur, {a.ds_y}, imgs, ACT_NONE);
            idt = {a.ds_y};
        }
        const Out out = last ? Out{a.out.f} : kept(a.out);
        LP(L); conv_fwd_eval(e, L, blk.c2, W, kept(a.z1), out, imgs, ACT_RELU, idt);
        cur = out;
    }
    const Conv& cl = e->convs[e->blocks.back().c2];
    LP(L); k_avgpool(cur.f, DT_F32, feat, imgs, cl.hout * cl.wout, 512, L.st);
    LP(L); k_fc_fwd(feat, S + e->off_fcw, S + e->off_fcb, logits, imgs, 512, e->C, L.st);
}

// d loss / d image of `imgs` images from the gradient of the stem's raw output (stem_dgrad.hip): dy [imgs][hout][wout][cout_p] in
// the engine's storage type, dx fp32 NCHW (NHWC through fm_debug_conv).  Written, not accumulated.
// The stem's data-gradient matrix is allocated at its first use (stale from the start: nothing clears its flag before)
int ensure_stem_dpack(fm_engine* e)
{
    if (e->model != 0) return FM_OK;
    const Conv& c0 = e->convs[0];
    if (!e->stem_dpack) DALLOC(e->stem_dpack, stem_dgrad_pack_floats());
    if (e->stem_dpack_stale) k_stem_dgrad_pack(e->student.state + c0.w_off, e->stem_dpack, c0.Kw, c0.kw_p, c0.cin_p, e->main.st);
    e->stem_dpack_stale = false;
    return FM_OK;
}
void stem_dgrad(fm_engine* e, Lane& L, const void* dy, float* dx, int imgs, bool nhwc)
{
    const Conv& c = e->convs[e->model == 1 ? e->c_stem : 0];
    if (e->model == 1)
        k_eff_stem_dgrad(dy, e->dt, e->student.state + c.w_off, dx, imgs, c.hin, c.win, c.hout, c.wout, c.pad, c.pad, c.Kw, c.kw_p, c.cin_p,
                         nhwc, L.st);
    else k_stem_dgrad((const float*)dy, e->stem_dpack, dx, imgs, c.hout, c.wout, c.hin, c.win, nhwc, L.st);
}
// the views' input gradients the backward was asked for (fm_backward_grads_x), from the stem's complete dy
void stem_dgrad_views(fm_engine* e, Lane& L, const void* dy, int groups, int B, float* const* dx)
{
    const Conv& c = e->convs[e->model == 1 ? e->c_stem : 0];
    const size_t view_bytes = (size_t)B * c.hout * c.wout * c.cout_p * (e->dt == DT_BF16 ? 2 : 4);
    for (int g = 0; g < groups && g < 2; ++g)
        if (dx[g]) stem_dgrad(e, L, (const char*)dy + g * view_bytes, dx[g], B, false);
}

// what every optimizer step ends with: the student's weights moved on the main lane
void weights_stepped(fm_engine* e)
{
    net_changed(e, e->student);
    ensure_packed(e);        // the next step's data gradients read the packed (transposed) weights
}
// The scalars of step t of each rule (optim.hip), for the flat steps and, per group, the grouped ones: what torch forms in double
// is formed in double here, from the fp32 values of fm_adam / fm_sgd.
OptAdamHp adam_hp(const fm_adam& hp, int64_t t)
{
    const double bc1 = 1.0 - pow((double)hp.beta1, (double)t), bc2 = 1.0 - pow((double)hp.beta2, (double)t);
    return {hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, (float)bc1, (float)sqrt(bc2)};
}
OptAdamWHp adamw_hp(const fm_adam& hp, int64_t t)
{
    const double bc1 = 1.0 - pow((double)hp.beta1, (double)t), bc2 = 1.0 - pow((double)hp.beta2, (double)t);
    return {(float)(1.0 - (double)hp.lr * (double)hp.weight_decay), (float)((double)hp.lr / bc1), hp.beta2, hp.eps, (float)sqrt(bc2),
            1.0 - (double)hp.beta1};
}
// first: the first step after a reset (torch: the momentum buffer does not exist yet)
OptSgdHp sgd_hp(const fm_sgd& hp, bool first)
{
    return {(double)hp.lr, (double)hp.momentum, 1.0 - (double)hp.dampening, (double)hp.weight_decay,
            (hp.momentum != 0.f && hp.nesterov != 0) ? 1 : 0, hp.momentum == 0.f ? 0 : (first ? 1 : 2)};
}
// The gradient an optimizer step reads: g itself, or, while a client-drift correction is installed (fm_drift_begin), the
// corrected copy that one launch on the main lane writes in front of the optimizer kernel (drift.hip has the rule).  g is only
// read: the accumulator, fm_get_grads, the norm and the clips keep the raw gradient.  Under a requires_grad mask the table form
// runs (frozen entries: a zero gradient, no sum).  With nothing installed this is the branch below and nothing else.
OptSel mask_sel(const fm_engine* e, const int32_t* tr);
const float* drift_grad(fm_engine* e, const float* g)
{
    if (!e->drift_on) return g;
    OP(e->main, "drift_correct");
    const DriftOps a{g, e->student.state, e->drift_anchor, e->drift_shifted ? e->drift_shift : nullptr,
                     e->drift_track ? e->drift_gsum : nullptr, e->drift_gcorr, e->drift_mu};
    if (e->trainable.empty()) k_drift_correct(a, (int64_t)e->NP, e->main.st, e->dev_err);
    else k_drift_correct_masked(a, e->tab.d_chunks, e->tab.n_param_chunks, mask_sel(e, e->trainable.data()), e->main.st, e->dev_err);
    e->drift_steps += 1;
    return e->drift_gcorr;
}
// optimizer.step(): one kernel over the whole trainable arena.  torch Adam with coupled L2 and the handle's hyper-parameters:
// g = e->grad (fused steps) or the autograd path's accumulator (fm_adam_step)
void adam_step(fm_engine* e, const float* g)
{
    g = drift_grad(e, g);
    e->adam_t += 1;
    k_adam(e->student.state, g, e->adam_m, e->adam_v, (int64_t)e->NP, adam_hp(e->hp, e->adam_t), e->main.st, e->dev_err);
    weights_stepped(e);
}
// torch.optim.AdamW / torch.optim.SGD over the autograd path's accumulator, with the handle's moment arenas and step count
void adamw_step(fm_engine* e, const fm_adam& hp)
{
    const float* g = drift_grad(e, e->gacc);
    e->adam_t += 1;
    k_adamw(e->student.state, g, e->adam_m, e->adam_v, (int64_t)e->NP, adamw_hp(hp, e->adam_t), e->main.st, e->dev_err);
    weights_stepped(e);
}
void sgd_step(fm_engine* e, const fm_sgd& hp)
{
    const float* g = drift_grad(e, e->gacc);
    const bool first = e->adam_t == 0;
    e->adam_t += 1;
    k_sgd(e->student.state, g, e->adam_m, (int64_t)e->NP, sgd_hp(hp, first), e->main.st, e->dev_err);
    weights_stepped(e);
}
// both moment arenas and the step count: a fresh optimizer of any kind
int optim_reset(fm_engine* e)
{
    e->adam_t = 0;
    HIPCHK(hipMemsetAsync(e->adam_m, 0, e->NP * 4, e->main.st));
    HIPCHK(hipMemsetAsync(e->adam_v, 0, e->NP * 4, e->main.st));
    return FM_OK;
}
const char* sgd_bad(const fm_sgd* hp)
{
    if (!(hp->lr >= 0.f && hp->momentum >= 0.f && hp->weight_decay >= 0.f)) return "fm_sgd: lr, momentum and weight_decay must be >= 0";
    if (!(hp->dampening == hp->dampening)) return "fm_sgd: dampening is NaN";
    if (hp->nesterov && !(hp->momentum > 0.f && hp->dampening == 0.f)) return "fm_sgd: nesterov needs momentum > 0 and dampening = 0";
    return nullptr;
}
const char* adam_bad(const fm_adam* hp)
{
    if (!(hp->lr >= 0.f && hp->eps >= 0.f && hp->weight_decay >= 0.f)) return "fm_adam: lr, eps and weight_decay must be >= 0";
    if (!(hp->beta1 >= 0.f && hp->beta1 < 1.f && hp->beta2 >= 0.f && hp->beta2 < 1.f)) return "fm_adam: betas must be in [0, 1)";
    return nullptr;
}
// the L2 norm of the accumulator into *norm (device), deterministic two-stage sum (optim.hip)
int grad_norm(fm_engine* e, float* norm)
{
    if (!e->norm_part) {
        DALLOC(e->norm_part, (size_t)grad_norm_parts((int64_t)e->NP));
        DALLOC(e->norm_word, 4);
        HIPCHK(hipMemsetAsync(e->norm_word, 0, 16, e->main.st));
    }
    k_grad_norm(e->gacc, (int64_t)e->NP, e->norm_part, norm, e->main.st, e->dev_err);
    return FM_OK;
}

// ---- per-layer requires_grad, parameter groups ----------------------------------------------------------------------
// a state entry is a PARAMETER if it is a float entry inside the trainable arena (running statistics and counters are buffers)
inline bool is_param(const fm_engine* e, const StateEntry& en) { return en.kind != 2 && en.eng_off < e->NP; }
// The engine's entry / chunk table (arena_table.h has its layout and the contract): one descriptor per state entry in
// state_dict order; plain host code up to the upload.
int build_arena_table(fm_engine* e)
{
    ArenaTable& t = e->tab;
    std::vector<ArenaDesc> descs;
    for (const StateEntry& en : e->entries)
        descs.push_back({en.kind, (long long)en.eng_off, en.span(), en.Ipad, en.I, en.Wpad, en.KW, is_param(e, en)});
    if (const char* why = arena_table_build(descs, (long long)e->NP, (long long)e->NS, t)) { g_err = why; return FM_ERR_ARG; }
    for (size_t i = 0; i < e->entries.size(); ++i)
        if (is_param(e, e->entries[i])) t.ent_at[e->entries[i].eng_off] = (int)i;
    // every offset the backward asks ent_on() about must start a table entry: a layout change fails here, not by quietly
    // switching truncation and the skipped weight gradients off (checked before anything is allocated)
    std::vector<size_t> offs = {e->off_fcw, e->off_fcb};
    for (auto& c : e->convs) offs.push_back(c.w_off);
    for (auto& b : e->bns) { offs.push_back(e->off_gamma + b.ch_off); offs.push_back(e->off_beta + b.ch_off); }
    for (auto& m : e->mbs) { offs.push_back(m.dw_off); offs.push_back(m.w1_off); offs.push_back(m.b1_off); offs.push_back(m.w2_off); offs.push_back(m.b2_off); }
    for (size_t o : offs)
        if (!t.ent_at.count(o)) { g_err = "a layer's arena offset starts no state entry (optimizer entry table)"; return FM_ERR_ARG; }
    DALLOC(t.d_ent, t.ent.size()); DALLOC(t.d_chunks, t.chunks.size());
    HIPCHK(hipMemcpy(t.d_ent, t.ent.data(), t.ent.size() * sizeof(ArenaEntry), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.d_chunks, t.chunks.data(), t.chunks.size() * sizeof(ArenaChunk), hipMemcpyHostToDevice));
    return FM_OK;
}
// is the parameter that starts at arena offset `off` trainable under the mask `tr` (null: yes)
inline bool ent_on(const fm_engine* e, const int32_t* tr, size_t off)
{
    if (!tr) return true;
    const auto it = e->tab.ent_at.find(off);         // (build_arena_table checked that every offset asked about resolves)
    return it == e->tab.ent_at.end() || tr[it->second] != 0;
}
inline bool conv_on(const fm_engine* e, const int32_t* tr, int ci) { return ent_on(e, tr, e->convs[ci].w_off); }
inline bool bn_on(const fm_engine* e, const int32_t* tr, int bi)
{
    return ent_on(e, tr, e->off_gamma + e->bns[bi].ch_off) || ent_on(e, tr, e->off_beta + e->bns[bi].ch_off);
}
// the launch's selector: the parameter group of every parameter's table entry, OPT_SKIP where nobody steps it (no group, or
// frozen)
OptSel group_sel(const fm_engine* e)
{
    OptSel sel{};
    for (size_t i = 0; i < e->entries.size(); ++i) {
        if (!is_param(e, e->entries[i])) continue;
        const int t = e->tab.ent_of[i];
        const int g = e->group_of[i];
        const bool on = g >= 0 && (e->trainable.empty() || e->trainable[i] != 0);
        opt_sel_set(sel, t, on ? (unsigned)g : OPT_SKIP);
    }
    return sel;
}
// ... and the masked accumulate's: 0 = trainable, 1 = frozen
OptSel mask_sel(const fm_engine* e, const int32_t* tr)
{
    OptSel sel{};
    for (size_t i = 0; i < e->entries.size(); ++i)
        if (is_param(e, e->entries[i])) opt_sel_set(sel, e->tab.ent_of[i], tr[i] != 0 ? 0u : 1u);
    return sel;
}
// The grouped steps: hp[i] belongs to group i of fm_optim_groups' table, and each group's scalars come from the function the flat
// step calls (adam_hp / adamw_hp / sgd_hp).  One step count per engine, as there.
void adam_step_groups(fm_engine* e, const fm_adam* hp, int n)
{
    const float* g = drift_grad(e, e->gacc);
    e->adam_t += 1;
    OptAdamArgs a{};
    for (int i = 0; i < n; ++i) a.hp[i] = adam_hp(hp[i], e->adam_t);
    k_adam_groups(e->student.state, g, e->adam_m, e->adam_v, e->tab.d_chunks, e->tab.n_param_chunks, group_sel(e), a, e->main.st, e->dev_err);
    weights_stepped(e);
}
void adamw_step_groups(fm_engine* e, const fm_adam* hp, int n)
{
    const float* g = drift_grad(e, e->gacc);
    e->adam_t += 1;
    OptAdamWArgs a{};
    for (int i = 0; i < n; ++i) a.hp[i] = adamw_hp(hp[i], e->adam_t);
    k_adamw_groups(e->student.state, g, e->adam_m, e->adam_v, e->tab.d_chunks, e->tab.n_param_chunks, group_sel(e), a, e->main.st, e->dev_err);
    weights_stepped(e);
}
void sgd_step_groups(fm_engine* e, const fm_sgd* hp, int n)
{
    const float* g = drift_grad(e, e->gacc);
    const bool first = e->adam_t == 0;
    e->adam_t += 1;
    OptSgdArgs a{};
    for (int i = 0; i < n; ++i) a.hp[i] = sgd_hp(hp[i], first);
    k_sgd_groups(e->student.state, g, e->adam_m, e->tab.d_chunks, e->tab.n_param_chunks, group_sel(e), a, e->main.st, e->dev_err);
    weights_stepped(e);
}

// Weight gradients on the side lane (side_w; otherwise everything below is a no-op that hands back the main lane).  A weight
// gradient reads a gradient tensor the main lane's data-gradient chain has just produced, and nothing waits for it before Adam.
// The tensors are double-buffered by block parity: side_begin records "tensor k of parity par produced" on the main lane, makes
// the side lane wait for it and returns the lane to launch the weight gradient on; side_end records "consumed" behind it;
// side_guard makes the main lane wait for that before it overwrites the tensor two blocks later; side_join brings every
// weight gradient back to the main lane before the optimizer reads e->grad.
Lane& side_begin(fm_engine* e, int k, int par)
{
    if (!e->side_w) return e->main;
    soft(e, hipEventRecord(e->ev_p[k][par], e->main.st));
    soft(e, lane_wait(e, FM_WAIT_SIDE_BEGIN, e->side.st, e->ev_p[k][par]));
    return e->side;
}
void side_end(fm_engine* e, int k, int par)
{
    if (e->side_w) soft(e, hipEventRecord(e->ev_c[k][par], e->side.st));
}
void side_guard(fm_engine* e, int k, int par)
{
    if (e->side_w) soft(e, lane_wait(e, FM_WAIT_SIDE_GUARD, e->main.st, e->ev_c[k][par]));
}
void side_join(fm_engine* e)
{
    if (!e->side_w) return;
    soft(e, hipEventRecord(e->ev_wdone, e->side.st));
    soft(e, lane_wait(e, FM_WAIT_SIDE_JOIN, e->main.st, e->ev_wdone));
}
// One weight gradient on the side lane: the fork behind tensor k of parity par, its fm_profile_ops scope, `launch(lane)`, the
// "consumed" event.  forked: the backward's note that side_join has something to bring back
template <typename Launch>
void side_wgrad(fm_engine* e, bool& forked, int k, int par, const char* op, Launch&& launch)
{
    forked = true;
    Lane& SL = side_begin(e, k, par);
    { OP(SL, op); launch(SL); }
    side_end(e, k, par);
}

// backward from e->dlogits (and bw.dfeat) through the student's activation set, as forward_train left it, into e->grad on the
// main lane, the weight gradients on the side lane; then Adam unless bw.step is false (fm_backward_grads)
void backward_and_step(fm_engine* e, int groups, int B, const Bwd& bw)
{
    const int imgs = groups * B;
    Lane& L = e->main;
    const Acts& A = e->acts;
    const float* S = e->student.state;
    const Conv& cl = e->convs[e->blocks.back().c2];
    // Under a mask (bw.train): units in forward order are the stem (0), the BasicBlocks (1 + b) and fc (nb + 1); `first` is the
    // first one with a trainable parameter.  Without a wanted dx nothing of a unit before it is enqueued, and a frozen conv's
    // weight gradient is not launched (nor its side-lane fork opened).  No mask: first = 0, every flag true, the list below
    // is the one it always was.
    const int32_t* tr = bw.train;
    const int nb = (int)e->blocks.size();
    int first = 0;
    if (tr && !(bw.dx[0] || bw.dx[1])) {
        auto blk_live = [&](const Block& k) {
            return conv_on(e, tr, k.c1) || bn_on(e, tr, k.c1) || conv_on(e, tr, k.c2) || bn_on(e, tr, k.c2) ||
                   (k.ds >= 0 && (conv_on(e, tr, k.ds) || bn_on(e, tr, k.ds)));
        };
        first = nb + 2;
        if (ent_on(e, tr, e->off_fcw) || ent_on(e, tr, e->off_fcb)) first = nb + 1;
        for (int b = nb - 1; b >= 0; --b)
            if (blk_live(e->blocks[b])) first = 1 + b;
        if (conv_on(e, tr, 0) || bn_on(e, tr, 0)) first = 0;
    }
    bool forked = false;               // a weight gradient went to the side lane: join it at the end
    if (first > nb + 1) return;        // nothing is trainable and no dx is wanted
    e->ctx = 500;
    { OP(L, "k_fc_bwd"); k_fc_bwd(e->dlogits, e->feat, S + e->off_fcw, nullptr, e->grad + e->off_fcw, e->grad + e->off_fcb, e->GA, DT_F32, imgs,
             512, e->C, cl.hout * cl.wout, L.st, bw.dfeat); }
    float *ga = e->GA, *ge = e->GE;
    for (int b = nb - 1; b >= 0 && 1 + b >= first; --b) {
        const Block& blk = e->blocks[b];
        e->ctx = 400 + b;                          // backward ops @400..@407 (fc @500, stem @399), like EfficientNet's
        const BlockActs& a = A.blk[b];
        const int par = b & 1;
        // side_w (stream_mode 0): d y2, d y_ds, d y1 double-buffered by block parity for the weight gradients on the side lane.
        // planes mode: they exist only as planes (read by the data gradients and the weight gradients) -- d y1's fp32 buffer still
        // takes d z1, the data gradient of conv 2
        const ResGrads& g = e->rg[par];
        const Out dy2 = kept(g.dy2), dyd = kept(g.dyd), dy1 = kept(g.dy1);
        const In in = b == 0 ? In(A.p0) : In(A.blk[b - 1].out);
        // out = relu(bn2(y2) + identity): masked grad dyh goes to bn2 and to the identity path.  The ReLU mask of an `out` kept as
        // planes is the sign of its h plane (the last block's `out` is fp32: it feeds the average pool)
        const bool last = b + 1 == (int)e->blocks.size();
        const In zo = last ? In{a.out.f} : In(kept(a.out));
        side_guard(e, 0, par);
        { OP(L, "bn_bwd"); bn_bwd(e, L, blk.c2, ga, dy2, groups, B, bw.frozen, zo.f ? Mask::Z : Mask::ZPlane, zo, ga); }
        if (blk.ds >= 0) { side_guard(e, 1, par); OP(L, "bn_bwd"); bn_bwd(e, L, blk.ds, ga, dyd, groups, B, bw.frozen); }
        // Where a weight gradient enters the side stream (round 6): behind the data gradient of the same conv, i.e. beside the
        // NEXT BatchNorm-backward passes of the main stream: a streaming kernel lives beside a GEMM's waves on a CU (the GEMMs leave
        // it the registers since their K-steps run row-major), two GEMMs do not (LDS).  Entering as soon as its dy exists put two
        // GEMMs beside each other and left the BatchNorm-backward passes that follow with nothing beside them.
        side_guard(e, 2, par);
        { OP(L, "conv_dgrad"); conv_dgrad(e, L, blk.c2, dy2, g.dy1.f, imgs); }
        if (conv_on(e, tr, blk.c2))
            side_wgrad(e, forked, 0, par, "conv_wgrad", [&](Lane& SL) { conv_wgrad(e, SL, blk.c2, kept(a.z1), dy2, imgs); });
        // z1 = relu(bn1(y1)): the mask comes from y1
        { OP(L, "bn_bwd"); bn_bwd(e, L, blk.c1, g.dy1.f, dy1, groups, B, bw.frozen, Mask::OwnOutput, kept(a.z1)); }
        // (the block the backward stops behind keeps its own data gradient: a unit runs whole or not at all)
        { OP(L, "conv_dgrad");
          if (blk.ds < 0) conv_dgrad(e, L, blk.c1, dy1, ge, imgs, {.res = ga});
          else if (!block_dgrad(e, L, blk.c1, blk.ds, dy1, dyd, ge, imgs)) {     // one launch: four classes + the downsample
              conv_dgrad(e, L, blk.ds, dyd, ge, imgs);                          // writes parity class (0,0)
              conv_dgrad(e, L, blk.c1, dy1, ge, imgs, {.acc_cls0 = true});      // all classes, (0,0) accumulates
          } }
        if (conv_on(e, tr, blk.c1))
            side_wgrad(e, forked, 2, par, "conv_wgrad", [&](Lane& SL) { conv_wgrad(e, SL, blk.c1, in, dy1, imgs); });
        if (blk.ds >= 0 && conv_on(e, tr, blk.ds))
            side_wgrad(e, forked, 1, par, "conv_wgrad", [&](Lane& SL) { conv_wgrad(e, SL, blk.ds, in, dyd, imgs); });
        std::swap(ga, ge);
    }
    const Conv& c0 = e->convs[0];
    e->ctx = 399;
    if (first == 0) {
        // max-pool backward + BatchNorm backward of the stem in two passes, without the dense intermediate (elementwise.hip)
        OP(L, "stem_pool_bn_bwd");
        Bn& b0 = e->bns[0];
        const BnSlots s0 = bn_slots(e, b0);
        const int pooled_pg = B * (c0.hout / 2) * (c0.wout / 2), pix = B * c0.hout * c0.wout;
        k_stem_pool_bn_reduce(ga, A.p0.f, e->idx0, c0.y, b0.mean, b0.istd, e->ws_part, groups, B, c0.hout, c0.wout, 64, L.st, s0.gamma,
                              s0.beta);
        bn_bwd_finalize(e, L, b0, groups, stem_pool_bn_blocks(pooled_pg), pix, bw.frozen);
        k_stem_pool_bn_apply(ga, A.p0.f, e->idx0, c0.y, e->ca, e->cb, e->cc, e->dyh0, groups, B, c0.hout, c0.wout, 64, L.st);
    }
    if (first == 0) {
        if (bw.dx[0] || bw.dx[1]) { OP(L, "stem_dgrad"); stem_dgrad_views(e, L, e->dyh0, groups, B, bw.dx); }
        if (conv_on(e, tr, 0)) { OP(L, "conv_wgrad"); conv_wgrad(e, L, 0, {e->x4}, {e->dyh0}, imgs); }
    }
    if (forked) side_join(e);
    if (bw.step) adam_step(e, e->grad);      // optimizer.step()
}

// =============================== EfficientNet-B0 graph =================================
// Squeeze-excite gate on the project conv's operand load: only where the conv reads its input once or twice
// (<= 2 M-tiles).  The late blocks (K = 672, 1152: 32-row M-tiles, 6-10 of them) would redo the BN + Swish
// prologue per M-tile on tensors that are tiny anyway: they keep the materialised a_s.
// fp32 storage: where the project conv's backward is fused (pw_proj_bwd_f32_kernel needs no a_s) and the train forward streams
// through conv1x1.hip, which then applies BN1 + Swish + gate on its operand load.
bool fuse_for(fm_engine* e, const MBConv& m)
{
    if (e->precision) return e->fuse_gate && pw_tiles_m(m.cout_p, m.ce_p) <= 2;
    return pw_proj_bwd_f32_nch(m.ce_p, m.cout_p, 1, m.hout * m.wout) > 0 && conv1x1_stream_takes(m.ce_p, m.cout_p, m.cout_p);
}

// BN over an arbitrary NHWC tensor (depthwise output): statistics by chan_reduce, then the same finalize
// partials: ws_part already holds that many partial sums per group (left by the depthwise forward); 0 = reduce here
void bn_fwd_tensor(fm_engine* e, Lane& L, int bi, const float* y, int groups, int pix_per_group, int HW, BnMode mode, int partials)
{
    if (!partials && mode != BnMode::Frozen)       // (frozen statistics need no statistics pass either)
        k_chan_reduce(nullptr, e->dt, y, e->dt, nullptr, nullptr, nullptr, nullptr, nullptr, e->ws_part, groups, pix_per_group,
                      HW, e->bns[bi].C, 0, 0, nullptr, nullptr, L.st);
    bn_fwd_stats(e, L, bi, e->ws_part, groups, partials ? partials : bn_bwd_blocks(pix_per_group), pix_per_group, mode, nullptr);
}

// what bnact_bwd's tensor carries beyond act(bn(y)).  rowscale: z = act(bn(y)) * rowscale[image]; gate / dsv: the squeeze-excite
// gate and pooled gradient, d a_d = dz * gate + dsv / HW formed on load; partials: ws_part already holds the two backward sums as
// that many partials per group (k_se_bwd_bn1, the depthwise data gradient), 0 = reduce here
struct BnActOps { const float *rowscale = nullptr, *gate = nullptr, *dsv = nullptr; int partials = 0; };
// backward through act(bn(y)): dz -> dy (may alias dz); writes dgamma/dbeta
void bnact_bwd(fm_engine* e, Lane& L, int bi, const float* dz, const float* y, float* dy, int groups, int pix_per_group, int HW, int act,
               bool frozen, const BnActOps& o = {})
{
    Bn& b = e->bns[bi];
    if (!o.partials)
        k_chan_reduce(dz, e->dt, y, e->dt, b.mean, b.istd, b.scale, b.shift, o.rowscale, e->ws_part, groups, pix_per_group, HW, b.C,
                      1, act, o.gate, o.dsv, L.st);
    bn_bwd_finalize(e, L, b, groups, o.partials ? o.partials : bn_bwd_blocks(pix_per_group), pix_per_group, frozen);
    k_bnact_bwd_apply(dz, e->dt, y, e->dt, e->ca, e->cb, e->cc, b.scale, b.shift, o.rowscale, dy, groups, pix_per_group, HW,
                      b.C, act, o.gate, o.dsv, L.st);
}

void eff_forward_train(fm_engine* e, Lane& L, Acts& A, int groups, int B, BnMode mode)
{
    const int imgs = groups * B;
    const Weights& W = e->student;
    const float* S = W.state;
    Conv& cs = e->convs[e->c_stem];
    e->ctx = -1;
    conv_fwd_train(e, L, e->c_stem, W, {e->x4}, groups, B, mode, "conv_fwd");
    {
        Bn& b = e->bns[e->bn_stem];
        { OP(L, "k_bnact_apply"); k_bnact_apply(cs.y, e->dt, b.scale, b.shift, nullptr, nullptr, A.a0, e->dt, groups, B * cs.hout * cs.wout,
                      cs.hout * cs.wout, b.C, 2, L.st); }
    }
    const float* cur = A.a0;
    for (size_t i = 0; i < e->mbs.size(); ++i) {
        const MBConv& m = e->mbs[i];
        MBActs& a = A.mb[i];
        e->ctx = (int)i;
        const int HWi = m.hin * m.win, HWo = m.hout * m.wout;
        const float* a_e = cur;
        if (m.c_exp >= 0) {
            Conv& ce = e->convs[m.c_exp];
            conv_fwd_train(e, L, m.c_exp, W, {cur}, groups, B, mode, "exp_fwd");
            Bn& b = e->bns[m.bn0];
            { OP(L, "k_bnact_apply"); k_bnact_apply(ce.y, e->dt, b.scale, b.shift, nullptr, nullptr, a.a_e, e->dt, groups, B * HWi, HWi, b.C, 2, L.st); }
            a_e = a.a_e;
        }
        bool st_done;
        { OP(L, "k_dw_fwd"); st_done = k_dw_fwd(a_e, S + m.dw_off, a.y_d, e->dt, nullptr, nullptr, imgs, m.hin, m.win, m.hout, m.wout, m.ce_p,
                 m.k, m.s, m.pad_t, m.pad_l, 0, L.st, L.rec, e->ws_part, groups); }   // + BN1 batch statistics
        { OP(L, "bn_fwd_tensor"); bn_fwd_tensor(e, L, m.bn1, a.y_d, groups, B * HWo, HWo, mode, st_done ? dw_stats_tiles() : 0); }
        {
            // a_d = swish(bn1(y_d)) is never written: the pooling and the gating pass form it on load
            Bn& b = e->bns[m.bn1];
            { OP(L, "k_se_fwd"); k_se_fwd(a.y_d, e->dt, b.scale, b.shift, B, A.se_pool, S + m.w1_off, S + m.b1_off, S + m.w2_off, S + m.b2_off,
                     a.sq, a.rpre, a.gate, imgs, HWo, m.ce_p, m.cs, L.st); }
            if (!fuse_for(e, m)) k_se_scale(a.y_d, e->dt, b.scale, b.shift, B, a.gate, a.a_s, imgs, HWo, m.ce_p, L.st);
        }
        Conv& cp = e->convs[m.c_proj];
        // a_s = swish(bn1(y_d)) * gate is formed on the project conv's operand load where it fuses
        if (fuse_for(e, m))
            conv_fwd_train(e, L, m.c_proj, W, {a.y_d}, groups, B, mode, "proj_fwd", {e->bns[m.bn1].scale, e->bns[m.bn1].shift, a.gate});
        else conv_fwd_train(e, L, m.c_proj, W, {a.a_s}, groups, B, mode, "proj_fwd");
        {
            Bn& b = e->bns[m.bn2];
            const float* dc = (m.skip && e->dc_dev) ? e->dc_dev + i * (size_t)imgs : nullptr;
            { OP(L, "k_bnact_apply"); k_bnact_apply(cp.y, e->dt, b.scale, b.shift, m.skip ? cur : nullptr, dc, a.out, e->dt, groups, B * HWo, HWo,
                          b.C, 0, L.st); }
        }
        cur = a.out;
    }
    Conv& ch = e->convs[e->c_head];
    const int HWh = ch.hout * ch.wout;
    e->ctx = 100;
    conv_fwd_train(e, L, e->c_head, W, {cur}, groups, B, mode, "conv_fwd");
    {
        Bn& b = e->bns[e->bn_head];
        { OP(L, "k_bnact_apply"); k_bnact_apply(ch.y, e->dt, b.scale, b.shift, nullptr, nullptr, A.T_mid, e->dt, groups, B * HWh, HWh, b.C, 2, L.st); }
    }
    { OP(L, "k_avgpool"); k_avgpool(A.T_mid, e->dt, e->feat, imgs, HWh, e->D, L.st); }
    const float* h = e->feat;
    if (e->drop_dev) {
        { OP(L, "k_mul"); k_mul(e->feat, e->drop_dev, e->hfeat, (int64_t)imgs * e->D, L.st); }
        h = e->hfeat;
    }
    { OP(L, "k_fc_fwd"); k_fc_fwd(h, S + e->off_fcw, S + e->off_fcb, e->logits, imgs, e->D, e->C, L.st); }
    if (mode != BnMode::Frozen) net_changed(e, e->student, Moved::Stats);
}

void eff_forward_eval(fm_engine* e, Lane& L, Weights& W, Acts& A, int imgs, float* feat, float* logits)
{
    const float* S = W.state;
    if (W.ev_dirty) { OP(L, "k_bn_eval_affine"); ensure_eval_affine(e, L, W); }
    auto sc = [&](int bi) { return W.ev_scale + e->bns[bi].ch_off; };
    auto sh = [&](int bi) { return W.ev_shift + e->bns[bi].ch_off; };
    { OP(L, "conv_fwd"); conv_fwd_eval(e, L, e->c_stem, W, {e->x4}, {A.a0}, imgs, ACT_SWISH); }
    const float* cur = A.a0;
    for (size_t i = 0; i < e->mbs.size(); ++i) {
        const MBConv& m = e->mbs[i];
        MBActs& a = A.mb[i];
        e->ctx = 201 + (int)i;                     // eval-mode ops are labelled @201..@216 (head @300)
        const int HWo = m.hout * m.wout;
        const float* a_e = cur;
        if (m.c_exp >= 0) {
            { OP(L, "exp_fwd"); conv_fwd_eval(e, L, m.c_exp, W, {cur}, {a.a_e}, imgs, ACT_SWISH); }
            a_e = a.a_e;
        }
        bool pooled;                      // eval: y_d holds swish(bn1(.)) directly; its per-image channel sums come with it
        { OP(L, "k_dw_fwd"); pooled = k_dw_fwd(a_e, S + m.dw_off, a.y_d, e->dt, sc(m.bn1), sh(m.bn1), imgs, m.hin, m.win, m.hout, m.wout, m.ce_p,
                 m.k, m.s, m.pad_t, m.pad_l, 2, L.st, L.rec, nullptr, 1, A.se_pool); }
        { OP(L, "k_se_fwd"); k_se_fwd(a.y_d, e->dt, nullptr, nullptr, 1, A.se_pool, S + m.w1_off, S + m.b1_off, S + m.w2_off, S + m.b2_off, a.sq,
                 a.rpre, a.gate, imgs, HWo, m.ce_p, m.cs, L.st, pooled); }
        // the gate multiplies the activation on the project conv's operand load: bf16 wherever the conv reads it once or twice,
        // fp32 where the conv streams through conv1x1.hip (K <= 256: the high-resolution blocks)
        const Conv& cpj = e->convs[m.c_proj];
        const In skip{m.skip ? cur : nullptr};         // the block's residual
        if (fuse_for(e, m) || (!e->precision && conv1x1_stream_takes(cpj.cin_p, cpj.cout_p, cpj.cout_p))) {
            { OP(L, "proj_fwd"); conv_fwd_eval(e, L, m.c_proj, W, {a.y_d}, {a.out}, imgs, ACT_NONE, skip, {.gate = a.gate}); }
        } else {
            { OP(L, "k_se_scale"); k_se_scale(a.y_d, e->dt, nullptr, nullptr, 1, a.gate, a.a_s, imgs, HWo, m.ce_p, L.st); }
            { OP(L, "proj_fwd"); conv_fwd_eval(e, L, m.c_proj, W, {a.a_s}, {a.out}, imgs, ACT_NONE, skip); }
        }
        cur = a.out;
    }
    Conv& ch = e->convs[e->c_head];
    e->ctx = 300;
    { OP(L, "conv_fwd"); conv_fwd_eval(e, L, e->c_head, W, {cur}, {A.T_mid}, imgs, ACT_SWISH); }
    { OP(L, "k_avgpool"); k_avgpool(A.T_mid, e->dt, feat, imgs, ch.hout * ch.wout, e->D, L.st); }
    { OP(L, "k_fc_fwd"); k_fc_fwd(feat, S + e->off_fcw, S + e->off_fcb, logits, imgs, e->D, e->C, L.st); }
}


// per-channel BatchNorm vectors [groups][C] the fused backward launches of the early MBConv blocks read (the graph's and the test
// hooks'): the forward's scale / shift (and mean / istd) and the backward's coefficients ca / cb / cc
struct BnCoef { const float *sc, *sh, *mean, *istd, *ca, *cb, *cc; };

// early blocks (62 % of the expanded-tensor bytes): BN0-backward apply + weight gradient + data gradient of the expand conv in ONE
// kernel that reads d a_e and y_e once (pw_exp_bwd_kernel / pw_exp_bwd_f32_kernel) instead of five passes over them
static bool exp_bwd_fuses(const Conv& c) { return (c.cout_p == 96 || c.cout_p == 144) && c.cin_p <= 32; }
// operands in the handle's storage type; returns the slabs written to L.ws_slab (reduce with k_reduce_slabs), 0 = shape not handled
static int launch_exp_bwd(fm_engine* e, Lane& L, const Conv& c, const void* dA, const void* Ye, const void* X, const void* res, void* dX,
                          const BnCoef& bn, int imgs, int groups)
{
    if (!exp_bwd_fuses(c)) return 0;
    PwExpBwdParams qb{};
    PwExpBwdF32Params qf{};
    auto fill = [&](auto& q) {             // the twin blocks differ in the element type and in the weight operand
        using T = std::remove_pointer_t<decltype(q.dX)>;
        q.dA = static_cast<const T*>(dA); q.Ye = static_cast<const T*>(Ye); q.X = static_cast<const T*>(X);
        q.res = static_cast<const T*>(res); q.dX = static_cast<T*>(dX);
        q.slab = L.ws_slab; q.ca = bn.ca; q.cb = bn.cb; q.cc = bn.cc; q.sc = bn.sc; q.sh = bn.sh;
        q.L = c.cout_p; q.S = c.cin_p; q.groups = groups;
        q.npix = imgs * c.hout * c.wout; q.pix_per_group = (imgs / groups) * c.hout * c.wout;
    };
    if (e->precision) { fill(qb); qb.Wt = e->student.wb + c.wbt_off; } else { fill(qf); qf.W = e->student.state + c.w_off; }
    return e->precision ? launch_pw_exp_bwd(qb, e->slab_floats, L.st) : launch_pw_exp_bwd_f32(qf, e->slab_floats, L.st);
}

// pooling records per image of the fused project backward of conv c; 0 = shape not handled
static int proj_bwd_nch(const fm_engine* e, const Conv& c, int imgs)
{
    const int HW = c.hout * c.wout;
    return e->precision ? pw_proj_bwd_nch(c.cin_p, c.cout_p, imgs, HW) : pw_proj_bwd_f32_nch(c.cin_p, c.cout_p, imgs, HW);
}
// phase 0: returns the slabs written to L.ws_slab (0 = not handled) and leaves the five per-image sums in the activation set's
// se_pool; phase 1: d y_d, 1 = launched.  ipg = images per statistics group, nch = proj_bwd_nch
static int launch_proj_bwd(fm_engine* e, Lane& L, const Conv& c, int phase, const void* dYp, const void* Yd, void* dYd,
                           const BnCoef& bn, const float* gate, const float* ds, int imgs, int ipg, int nch)
{
    PwProjBwdParams qb{};
    PwProjBwdF32Params qf{};
    auto fill = [&](auto& q) {
        using T = std::remove_pointer_t<decltype(q.dYd)>;
        q.dYp = static_cast<const T*>(dYp); q.Yd = static_cast<const T*>(Yd); q.dYd = static_cast<T*>(dYd);
        q.slab = L.ws_slab; q.pool5 = e->acts.se_pool;
        q.sc = bn.sc; q.sh = bn.sh; q.mean = bn.mean; q.istd = bn.istd; q.ca = bn.ca; q.cb = bn.cb; q.cc = bn.cc;
        q.gate = gate; q.ds = ds;
        q.L = c.cin_p; q.S = c.cout_p; q.imgs = imgs; q.HW = c.hout * c.wout; q.ipg = ipg; q.nch = nch;
    };
    if (e->precision) { fill(qb); qb.Wt = e->student.wb + c.wbt_off; } else { fill(qf); qf.W = e->student.state + c.w_off; }
    return e->precision ? launch_pw_proj_bwd(qb, phase, e->slab_floats, L.st) : launch_pw_proj_bwd_f32(qf, phase, e->slab_floats, L.st);
}

// same contract as backward_and_step
void eff_backward_and_step(fm_engine* e, int groups, int B, const Bwd& bw)
{
    const int imgs = groups * B;
    Lane& L = e->main;
    const Acts& A = e->acts;
    const float* S = e->student.state;
    float* G = e->grad;
    Conv& ch = e->convs[e->c_head];
    const int HWh = ch.hout * ch.wout;
    const float* h = e->drop_dev ? e->hfeat : e->feat;
    // Weight gradients on the side lane (side_wgrad): T_small (d y_p) for the project conv, T_mid (d y_d) for the depthwise
    // conv, T_big (d y_e) for the expand conv, the squeeze-excite vectors, each double-buffered by block parity (e->eg).  Arithmetic
    // and summation orders are those of the inline order: results are bit-identical.
    // Under a mask (bw.train; backward_and_step's note): units in forward order are the stem (0), the MBConv blocks (1 + i), the
    // head (nm + 1) and _fc (nm + 2).  Weight gradients that are launches of their own -- the pointwise and depthwise ones -- are
    // skipped for a frozen weight; those that come out of a kernel the data gradient needs (the fused expand / project backward,
    // BatchNorm's dgamma / dbeta, the squeeze-excite backward) are computed as ever and masked by the caller.
    const int32_t* tr = bw.train;
    const int nm = (int)e->mbs.size();
    int first = 0;
    if (tr && !(bw.dx[0] || bw.dx[1])) {
        auto mb_live = [&](const MBConv& m) {
            return (m.c_exp >= 0 && (conv_on(e, tr, m.c_exp) || bn_on(e, tr, m.bn0))) || ent_on(e, tr, m.dw_off) || bn_on(e, tr, m.bn1) ||
                   ent_on(e, tr, m.w1_off) || ent_on(e, tr, m.b1_off) || ent_on(e, tr, m.w2_off) || ent_on(e, tr, m.b2_off) ||
                   conv_on(e, tr, m.c_proj) || bn_on(e, tr, m.bn2);
        };
        first = nm + 3;
        if (ent_on(e, tr, e->off_fcw) || ent_on(e, tr, e->off_fcb)) first = nm + 2;
        if (conv_on(e, tr, e->c_head) || bn_on(e, tr, e->bn_head)) first = nm + 1;
        for (int i = nm - 1; i >= 0; --i)
            if (mb_live(e->mbs[i])) first = 1 + i;
        if (conv_on(e, tr, e->c_stem) || bn_on(e, tr, e->bn_stem)) first = 0;
    }
    bool forked = false;
    if (first > nm + 2) return;        // nothing is trainable and no dx is wanted
    e->ctx = 500;
    { OP(L, "k_fc_bwd"); k_fc_bwd(e->dlogits, h, S + e->off_fcw, e->drop_dev, G + e->off_fcw, G + e->off_fcb, A.T_mid, e->dt, imgs, e->D, e->C,
             HWh, L.st, bw.dfeat); }
    if (first > nm + 1) return;        // head-only training: _fc's backward and nothing else
    { OP(L, "bnact_bwd"); bnact_bwd(e, L, e->bn_head, A.T_mid, ch.y, A.T_mid, groups, B * HWh, HWh, ACT_SWISH, bw.frozen); }
    if (conv_on(e, tr, e->c_head)) { OP(L, "conv_wgrad"); conv_wgrad(e, L, e->c_head, {A.mb.back().out}, {A.T_mid}, imgs); }
    if (first > nm) return;
    float *go = e->GA, *gi = e->GB;
    { OP(L, "conv_dgrad"); conv_dgrad(e, L, e->c_head, {A.T_mid}, go, imgs); }
    for (int i = nm - 1; i >= 0 && 1 + i >= first; --i) {
        const MBConv& m = e->mbs[i];
        const MBActs& a = A.mb[i];
        e->ctx = 400 + i;                          // backward ops @400..@415 (head @500, stem @399)
        const int par = i & 1;
        const EffGrads& g = e->eg[par];
        float *T_small = g.dyp, *T_mid = g.dyd, *T_big = g.dye;
        float *dgp = g.se_dg, *drp = g.se_dr;          // the squeeze-excite gradient vectors alternate too
        const float* in = i == 0 ? A.a0 : A.mb[i - 1].out;
        const int HWi = m.hin * m.win, HWo = m.hout * m.wout;
        Conv& cp = e->convs[m.c_proj];
        const float* dc = (m.skip && e->dc_dev) ? e->dc_dev + (size_t)i * imgs : nullptr;
        // out = bn2(y_p)*dc + in
        side_guard(e, 0, par);
        { OP(L, "bnact_bwd"); bnact_bwd(e, L, m.bn2, go, cp.y, T_small, groups, B * HWo, HWo, ACT_NONE, bw.frozen, {.rowscale = dc}); }
        Bn& b1 = e->bns[m.bn1];
        // early blocks (half of the depthwise-resolution bytes): d a_s is never stored -- pw_proj_bwd_kernel forms it twice on the
        // matrix pipe, once for the five per-image sums + the weight gradient, once for the BN1-backward apply (7 passes -> 3)
        const int nch5 = proj_bwd_nch(e, cp, imgs);
        // the squeeze-excite backward: ONE pass over (d a_s, y_d) -- or, behind the fused sums, over their nch pooling records with
        // d a_s null -- yields its pooled sums and the BN1-backward sums; its weight gradient on side lane 3
        auto se_bwd = [&](const float* das, int nch) {
            side_guard(e, 3, par);
            { OP(L, "k_se_bwd"); k_se_bwd_bn1(das, a.y_d, e->dt, b1.scale, b1.shift, b1.mean, b1.istd, B, A.se_pool, a.gate, a.rpre,
                         S + m.w1_off, S + m.w2_off, dgp, drp, e->se_ds, e->ws_part, imgs, HWo, m.ce_p, m.cs, L.st, nch); }
            side_wgrad(e, forked, 3, par, "k_se_wgrad", [&](Lane& SL) {
                k_se_wgrad(dgp, drp, a.rpre, a.sq, SL.ws_slab, G + m.w1_off, imgs, m.ce_p, m.cs, SL.st); });
        };
        bool pfused = false;
        if (nch5) {
            auto launch = [&](int phase) {
                return launch_proj_bwd(e, L, cp, phase, T_small, a.y_d, T_mid, {b1.scale, b1.shift, b1.mean, b1.istd, e->ca, e->cb, e->cc},
                                       a.gate, e->se_ds, imgs, B, nch5);
            };
            int sk;
            { OP(L, "proj_bwd_sums"); sk = launch(0);
              if (sk > 0) k_reduce_slabs(L.ws_slab, G + cp.w_off, sk, (int64_t)cp.w_numel, L.st); }
            if (sk > 0) {
                se_bwd(nullptr, nch5);
                side_guard(e, 1, par);
                { OP(L, "proj_bwd_apply");
                  bn_bwd_finalize(e, L, b1, groups, se_bwd_bn1_splits(B), B * HWo, bw.frozen);
                  if (launch(1) != 1) soft(e, hipErrorInvalidValue); }      // d y_d
                pfused = true;
            }
        }
        if (!pfused) {
            if (!e->precision && fuse_for(e, m)) soft(e, hipErrorInvalidValue);     // fp32: a_s was not stored for this block and only
                                                                                    // the fused backward can do without it
            if (conv_on(e, tr, m.c_proj))
                side_wgrad(e, forked, 0, par, "proj_wgrad", [&](Lane& SL) {
                    // where the project conv's operand a_s was never stored it is re-formed from y_d on load
                    if (fuse_for(e, m)) conv_wgrad(e, SL, m.c_proj, {a.y_d}, {T_small}, imgs, {b1.scale, b1.shift, a.gate}, B * HWo);
                    else conv_wgrad(e, SL, m.c_proj, {a.a_s}, {T_small}, imgs);
                });
            side_guard(e, 1, par);
            { OP(L, "proj_dgrad"); conv_dgrad(e, L, m.c_proj, {T_small}, T_mid, imgs); }          // d a_s
            se_bwd(T_mid, 0);                 // a_s = a_d * gate(a_d)
            // d a_d = d a_s * gate + ds/HW is formed on load inside the BN backward's apply pass
            { OP(L, "bnact_bwd"); bnact_bwd(e, L, m.bn1, T_mid, a.y_d, T_mid, groups, B * HWo, HWo, ACT_SWISH, bw.frozen,
                                         {.gate = a.gate, .dsv = e->se_ds, .partials = se_bwd_bn1_splits(B)}); }   // d y_d
        }
        const float* a_e = m.c_exp >= 0 ? a.a_e : in;
        if (ent_on(e, tr, m.dw_off))
            side_wgrad(e, forked, 1, par, "k_dw_wgrad", [&](Lane& SL) {
                k_dw_wgrad(T_mid, a_e, e->dt, SL.ws_slab, G + m.dw_off, imgs, m.hin, m.win, m.hout, m.wout, m.ce_p, m.k, m.s, m.pad_t,
                           m.pad_l, SL.st); });
        if (m.c_exp >= 0) {
            Conv& ce = e->convs[m.c_exp];
            Bn& b0 = e->bns[m.bn0];
            bool sums;                           // d a_e, and the BN0-backward sums from the same registers
            side_guard(e, 2, par);
            { OP(L, "k_dw_dgrad"); sums = k_dw_dgrad(T_mid, S + m.dw_off, T_big, e->dt, imgs, m.hin, m.win, m.hout, m.wout, m.ce_p, m.k, m.s,
                       m.pad_t, m.pad_l, L.st, ce.y, b0.mean, b0.istd, b0.scale, b0.shift, L.rec, e->ws_part, groups); }
            bool fused = false;
            if (exp_bwd_fuses(ce)) {
                OP(L, "exp_bwd_fused");
                const int pix = B * HWi;
                if (!sums)
                    k_chan_reduce(T_big, e->dt, ce.y, e->dt, b0.mean, b0.istd, b0.scale, b0.shift, nullptr, e->ws_part, groups, pix,
                                  HWi, b0.C, 1, 2, nullptr, nullptr, L.st);
                bn_bwd_finalize(e, L, b0, groups, sums ? dw_stats_tiles() : bn_bwd_blocks(pix), pix, bw.frozen);
                const int sk = launch_exp_bwd(e, L, ce, T_big, ce.y, in, m.skip ? go : nullptr, gi,
                                              {b0.scale, b0.shift, nullptr, nullptr, e->ca, e->cb, e->cc}, imgs, groups);
                if (sk > 0) {
                    k_reduce_slabs(L.ws_slab, G + ce.w_off, sk, (int64_t)ce.w_numel, L.st);
                    fused = true;
                }
            }
            if (!fused) {
                // (a refused fused launch has left ca / cb / cc and the BN gradients exactly as bnact_bwd is about to)
                { OP(L, "bnact_bwd"); bnact_bwd(e, L, m.bn0, T_big, ce.y, T_big, groups, B * HWi, HWi, ACT_SWISH, bw.frozen,
                                             {.partials = sums ? dw_stats_tiles() : 0}); }
                if (conv_on(e, tr, m.c_exp))
                    side_wgrad(e, forked, 2, par, "exp_wgrad", [&](Lane& SL) { conv_wgrad(e, SL, m.c_exp, {in}, {T_big}, imgs); });
                { OP(L, "exp_dgrad"); conv_dgrad(e, L, m.c_exp, {T_big}, gi, imgs, {.res = m.skip ? go : nullptr}); }
            }
        } else {
            { OP(L, "k_dw_dgrad"); k_dw_dgrad(T_mid, S + m.dw_off, gi, e->dt, imgs, m.hin, m.win, m.hout, m.wout, m.ce_p, m.k, m.s, m.pad_t,
                       m.pad_l, L.st); }
            if (m.skip) k_add_inplace(gi, go, e->dt, (int64_t)imgs * HWi * m.cin_p, L.st);
        }
        std::swap(go, gi);
    }
    Conv& cs = e->convs[e->c_stem];
    e->ctx = 399;
    if (first == 0) {
        { OP(L, "bnact_bwd"); bnact_bwd(e, L, e->bn_stem, go, cs.y, go, groups, B * cs.hout * cs.wout, cs.hout * cs.wout, ACT_SWISH, bw.frozen); }
        if (bw.dx[0] || bw.dx[1]) { OP(L, "stem_dgrad"); stem_dgrad_views(e, L, go, groups, B, bw.dx); }
        if (conv_on(e, tr, e->c_stem)) { OP(L, "conv_wgrad"); conv_wgrad(e, L, e->c_stem, {e->x4}, {go}, imgs); }
    }
    if (forked) side_join(e);                    // every weight gradient is in G before the optimizer reads it
    if (bw.step) { OP(L, "adam_step"); adam_step(e, e->grad); }
}

// model dispatch.  The train forward and the backward are the student's: main lane, the student's activation set
void net_forward_train(fm_engine* e, int groups, int B, BnMode mode = BnMode::Batch)
{
    ensure_packed(e);
    if (e->model == 1) eff_forward_train(e, e->main, e->acts, groups, B, mode);
    else forward_train(e, e->main, e->acts, groups, B, mode);
}
// W's shadows are the caller's to ensure (ensure_packed / ensure_fwd_shadows: main lane)
void net_forward_eval(fm_engine* e, Lane& L, Weights& W, Acts& A, int imgs, float* feat, float* logits)
{
    if (e->model == 1) eff_forward_eval(e, L, W, A, imgs, feat, logits);
    else forward_eval(e, L, W, A, imgs, feat, logits);
}
// the teacher's forward on the side lane, into the second activation set: the same code as on the main lane
int teacher_forward_side(fm_engine* e, int imgs)
{
    ensure_fwd_shadows(e, e->teacher);                          // weight shadows on the main lane, before the fork
    HIPCHK(hipEventRecord(e->ev_in, e->main.st));
    HIPCHK(lane_wait(e, FM_WAIT_EV_IN, e->side.st, e->ev_in));
    net_forward_eval(e, e->side, e->teacher, e->tacts, imgs, e->tfeat, e->tlogits);
    HIPCHK(hipEventRecord(e->ev_t, e->side.st));
    return FM_OK;
}
// the frozen teacher's eval forward of the staged batch (timgs images) beside the student's train forward of `groups` views of B: on
// the side lane with its own activation set (they meet at the loss), else first (its activations may be overwritten by the student)
int teacher_and_student_forward(fm_engine* e, int timgs, int groups, int B)
{
    if (e->side_ok) RCCHK(teacher_forward_side(e, timgs));
    else {
        ensure_fwd_shadows(e, e->teacher);
        net_forward_eval(e, e->main, e->teacher, e->acts, timgs, e->tfeat, e->tlogits);
    }
    net_forward_train(e, groups, B);
    if (e->side_ok) HIPCHK(lane_wait(e, FM_WAIT_EV_T, e->main.st, e->ev_t));
    return FM_OK;
}
void net_backward_and_step(fm_engine* e, int groups, int B, const Bwd& bw = {})
{
    ensure_packed(e);
    if (e->model == 1) eff_backward_and_step(e, groups, B, bw);
    else backward_and_step(e, groups, B, bw);
}

// an engine-layout arena -> dst in state_dict order (conv weights OIHW; e->nf_sd floats), enqueued on the main lane.  np_only: an
// arena of NP floats (e->grad, the accumulator, the moments): the BN running statistics come out as zeros
int arena_to_state_dict(fm_engine* e, const float* src, float* dst, bool np_only)
{
    Lane& L = e->main;
    size_t off = 0;
    for (auto& en : e->entries) {
        if (en.kind == 0) {
            k_ohwi_to_oihw(src + en.eng_off, dst + off, en.O, en.I, en.KH, en.KW, en.Wpad, en.Ipad, L.st, en.Ostride);
            off += en.n;
        } else if (en.kind == 1) {
            if (!np_only || en.eng_off < e->NP)
                HIPCHK(hipMemcpyAsync(dst + off, src + en.eng_off, en.n * 4, hipMemcpyDeviceToDevice, L.st));
            else
                HIPCHK(hipMemsetAsync(dst + off, 0, en.n * 4, L.st));
            off += en.n;
        }
    }
    return FM_OK;
}

// the inverse: src in state_dict order (device, e->nf_sd floats) -> an engine-layout arena, enqueued on the main lane.  The
// padding inside a conv's matrix is written as zeros; rows, tails and gaps outside it are not touched.  np_only: an arena of
// NP floats (the moments): the BN running statistics are passed over
int state_dict_to_arena(fm_engine* e, const float* src, float* arena, bool np_only)
{
    Lane& L = e->main;
    size_t off = 0;
    for (auto& en : e->entries) {
        if (en.kind == 0) {
            k_oihw_to_ohwi(src + off, arena + en.eng_off, en.O, en.I, en.KH, en.KW, en.Wpad, en.Ipad, L.st, en.Ostride);
            off += en.n;
        } else if (en.kind == 1) {
            if (!np_only || en.eng_off < e->NP)
                HIPCHK(hipMemcpyAsync(arena + en.eng_off, src + off, en.n * 4, hipMemcpyDeviceToDevice, L.st));
            off += en.n;
        }
    }
    return FM_OK;
}

// debug hooks: fold the per-tile partials conv `ci`'s forward left in ws_stats with the finalize kernel's own reduction order
// (sum / sumsq only) into stats_dev [groups][2][cout_p]
int debug_fold_stats(fm_engine* e, int ci, int groups, float* stats_dev)
{
    const int tiles = stats_tiles(e, ci), n = 2 * e->convs[ci].cout_p;
    std::vector<float> h((size_t)groups * tiles * n), o((size_t)groups * n, 0.f);
    HIPCHK(hipMemcpyAsync(h.data(), e->ws_stats, h.size() * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    for (int g = 0; g < groups; ++g)
        for (int k = 0; k < n; ++k) {
            double sum = 0;
            for (int t = 0; t < tiles; ++t) sum += h[((size_t)g * tiles + t) * n + k];
            o[(size_t)g * n + k] = (float)sum;
        }
    HIPCHK(hipMemcpy(stats_dev, o.data(), o.size() * 4, hipMemcpyHostToDevice));
    return FM_OK;
}

// the launch of fm_fedavg_fold / fm_fed_w: fp32 weights and the divisor as the caller formed them
int fold_states(fm_engine* e, const FoldArgs& a, int K, float tot, float* out_dev)
{
    k_fedavg_fold(a, K, tot, out_dev, (int64_t)e->NS, e->main.st);
    if (out_dev == e->student.state) net_changed(e, e->student);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

ClassVec to_cv(const float* h, int C)
{
    ClassVec v{};
    for (int i = 0; i < C; ++i) v.v[i] = h[i];
    return v;
}

}  // namespace

// what the fused steps answer under a non-default requires_grad mask
static const char* const kMaskRefusal =
    "a requires_grad mask is installed and the fused steps train every layer: use the autograd path (fm_forward_train, "
    "fm_backward_grads, fm_adam_step_groups / fm_adamw_step_groups / fm_sgd_step_groups), or restore the default mask with "
    "fm_set_trainable";

// ---- the fused training steps: one skeleton, and per loss head its argument rules (`*_bad`) and its launcher ----
namespace {

int count_active(const fm_engine* e, const float* active_mask_host)
{
    int n = 0;
    for (int c = 0; c < e->C; ++c) n += active_mask_host[c] != 0.f;
    return n;
}
// the single-view heads' common contract: at least one active and one missing class (torch forms 0/0 or the mean of an empty
// tensor otherwise)
const char* classes_bad(const fm_engine* e, const float* active_mask_host)
{
    const int na = count_active(e, active_mask_host);
    return na >= 1 && na < e->C ? nullptr : "the head needs at least one active and one missing class";
}
const char* norm_bad(int B, int ann, int bs)
{
    return B >= 1 && ann >= 1 && bs >= 1 && (int64_t)bs * ann < (1 << 24)
               ? nullptr : "B, annotation_num, bs_norm >= 1; bs_norm * annotation_num < 2^24";
}
const char* fedlsr_bad(float mix1, bool step)
{
    if (mix1 >= 0.f && mix1 <= 1.f) return nullptr;
    return step ? "fm_step_fedlsr: mix1 in [0, 1]" : "fm_loss_fedlsr: mix1 in [0, 1]";
}
const char* fedirm_bad(int B, int ann, int bs, bool rel)
{
    if (const char* bad = norm_bad(B, ann, bs)) return bad;
    return rel && B > 2048 ? "fm_loss_fedirm_rel: B <= 2048 (the selected-row table)" : nullptr;
}
const char* rscfed_bad(const fm_engine* e, const float* am, int ann, int bs, int B)
{
    if (const char* bad = norm_bad(B, ann, bs)) return bad;
    return classes_bad(e, am);
}
const char* cbafed_bad(const fm_engine* e, const float* am, int ann, int bs, const float* tao, const int64_t* counts_dev, int B,
                       bool step)
{
    if (tao && !counts_dev)
        return step ? "fm_step_cbafed: stage 2 (tao given) needs counts_dev" : "fm_loss_cbafed: stage 2 (tao given) needs counts_dev";
    return rscfed_bad(e, am, ann, bs, B);
}
// fm_loss_rofl / fm_step_rofl: what the host can check of the caller's arguments
const char* rofl_bad(const fm_engine* e, const void* feat, const void* item, const void* centroids, const void* pseudo, int B,
                     int n_keep, int64_t N)
{
    if (!feat || !item || !centroids || !pseudo) return "null";
    if (B < 1) return "B >= 1";
    if (B > e->maxB) return "B exceeds max_images";
    if (n_keep < 1) return "rofl: n_keep < 1 (int((1 - forget_rate) * B) of a batch this small keeps no row)";
    if (n_keep > B) return "rofl: n_keep > B";
    if (N < 1 || N * e->C > INT32_MAX) return "rofl: 1 <= N, N * n_classes < 2^31";
    if (e->D % 4 || ((uintptr_t)feat | (uintptr_t)centroids) % 16) return "rofl: feature and centroid rows must be 16-byte aligned";
    return nullptr;
}
// the RoFL workspaces, at the first call that needs them
int rofl_ws(fm_engine* e)
{
    if (e->rofl_keep) return FM_OK;
    DALLOC(e->rofl_rowloss, (size_t)e->maxB);
    DALLOC(e->rofl_dist, (size_t)e->maxB * e->C);
    DALLOC(e->rofl_cos, (size_t)e->maxB * 2 * e->C);
    DALLOC(e->rofl_keep, (size_t)e->maxB);
    return FM_OK;
}
void launch_rofl(fm_engine* e, const float* z, const float* feat, const float* y, const int32_t* item, int B, int n_keep,
                 const float* pw, float lambda_cen, float lambda_e, int write_labels, float* centroids, uint8_t* pseudo, int64_t N,
                 float* dz, float* loss, int32_t* keep)
{
    k_loss_rofl(z, feat, y, item, B, e->C, e->D, n_keep, to_cv(pw, e->C), lambda_cen, lambda_e, write_labels, centroids, pseudo,
                (int)N, e->rofl_rowloss, e->rofl_cos, e->rofl_dist, e->rofl_keep, keep, dz, loss, e->main.st);
}

void launch_fedlsr(fm_engine* e, const float* z, const float* y, const float* pw, float mix1, float beta, int B, float* dz, float* loss)
{
    k_loss_fedlsr(z, y, to_cv(pw, e->C), B, e->C, mix1, (float)(1.0 - (double)mix1), beta, dz, loss, e->main.st);
}
void launch_rscfed(fm_engine* e, const float* z, const float* zt, const float* y, const float* pw, const float* am, int ann, int bs,
                   int B, float* dz, float* loss)
{
    k_loss_rscfed(z, zt, y, to_cv(pw, e->C), to_cv(am, e->C), B, e->C, (float)bs * (float)ann, e->C - count_active(e, am), dz, loss,
                  e->main.st);
}
void launch_lakd(fm_engine* e, const float* z, const float* zt, const float* y, const float* am, float w_kd, int B, float* dz,
                 float* loss)
{
    k_loss_lakd(z, zt, y, to_cv(am, e->C), B, e->C, count_active(e, am), w_kd, dz, loss, e->main.st);
}
void launch_cbafed(fm_engine* e, const float* z, const float* y, const float* am, int ann, int bs, const float* tao, int B,
                   float* pw_dev, int64_t* counts_dev, float* dz, float* loss)
{
    ClassVec t{};
    if (tao) t = to_cv(tao, e->C);
    k_loss_cbafed(z, y, to_cv(am, e->C), tao ? &t : nullptr, B, e->C, (float)bs * (float)ann, ann, pw_dev, counts_dev, dz, loss,
                  e->main.st);
}

// which forwards a fused step runs before its head
enum class StepFwd {
    Student,     // the student's train forward of every staged view
    Frozen,      // the frozen teacher's eval forward of the staged batch beside it (teacher_and_student_forward)
    Rscfed       // the EMA teacher's eval forward of view 2 beside the student's train forward of view 1
};

// A fused step: refusals (nothing is enqueued before the last of them), staging of x1 (and x2), the forwards, `head` on e->logits
// (and e->tlogits) -> e->dlogits, backward and Adam.  head_bad is the head's `*_bad` answer for the caller's arguments.
// Rscfed's lane order: both views are staged on the main lane (view 2 as the staging's second group); the teacher's
// shadows are re-formed on the main lane, behind the previous step's blend; ev_in lets the side lane start, ev_t brings it back
// before the head -- so the blend, on the main lane behind Adam, never meets a running teacher forward, and the next step's fork is
// enqueued behind it.
template <typename Head>
int fused_step(fm_engine* e, StepFwd fwd, const float* x1, const float* x2, int B, const char* head_bad, Head head)
{
    const int views = x2 ? 2 : 1;                                 // staged
    const int groups = fwd == StepFwd::Rscfed ? 1 : views;        // trained on
    ARGCHK(e->trainable.empty(), kMaskRefusal);
    if (groups == 2) ARGCHK(B >= 1 && 2 * B <= e->maxB, "2*B exceeds max_images");
    else ARGCHK(B >= 1 && B <= e->maxB, "B exceeds max_images");
    BADCHK(head_bad);
    lane_point(e, 0);
    const float* xs[2] = {x1, x2};
    if (fwd == StepFwd::Rscfed && !(e->side_ok && 2 * B <= e->maxB)) {
        // one lane (or no room for both views in the staging): the teacher first, each view staged in turn
        to_nhwc4(e, e->main, &x2, 1, B);
        ensure_fwd_shadows(e, e->teacher);
        net_forward_eval(e, e->main, e->teacher, e->acts, B, e->tfeat, e->tlogits);
        to_nhwc4(e, e->main, &x1, 1, B);
        net_forward_train(e, 1, B);
    } else {
        to_nhwc4(e, e->main, xs, views, B);
        if (fwd == StepFwd::Student) net_forward_train(e, groups, B);
        else if (fwd == StepFwd::Frozen) RCCHK(teacher_and_student_forward(e, views * B, groups, B));
        else {
            e->in_img0 = B;                      // the teacher's stem reads the second group
            const int rc = teacher_forward_side(e, B);
            e->in_img0 = 0;
            RCCHK(rc);
            net_forward_train(e, 1, B);
            HIPCHK(lane_wait(e, FM_WAIT_EV_T, e->main.st, e->ev_t));
        }
    }
    head();
    net_backward_and_step(e, groups, B);
    STEP_DONE(e);
    return FM_OK;
}

}  // namespace

// =============================== C ABI =======================================
extern "C" {

int fm_create(const fm_config* cfg, fm_engine** out)
{
    ARGCHK(cfg && out, "null cfg/out");
    ARGCHK(cfg->model == 0 || cfg->model == 1, "model must be 0 (ResNet-18) or 1 (EfficientNet-B0)");
    ARGCHK(cfg->n_classes >= 1 && cfg->n_classes <= FM_MAX_CLASSES, "n_classes out of range");
    ARGCHK(cfg->in_h >= 32 && cfg->in_w >= 32 && cfg->in_h % 32 == 0 && cfg->in_w % 32 == 0,
           "in_h/in_w must be multiples of 32");
    ARGCHK(cfg->max_images >= 1, "max_images");
    ARGCHK(cfg->reserved[0] == 0 || (cfg->reserved[0] == 1 && cfg->model == 1),
           "precision (reserved[0]) must be 0 (fp32) or, for EfficientNet-B0, 1 (bf16 activations)");
    ARGCHK(cfg->reserved[1] >= 0 && cfg->reserved[1] <= 2, "reserved[1] (stream mode) must be 0, 1 or 2");
    ARGCHK(cfg->reserved[2] >= 0 && cfg->reserved[2] <= 3,
           "reserved[2] (product form of the fp32 conv GEMMs) must be 0 (library default: six bf16 partial products), 1 (fp32 "
           "matrix pipe), 2 (nine bf16 partial products) or 3 (exactly six, whatever the default)");
    fm_engine* e = new fm_engine();
    e->precision = cfg->reserved[0];
    e->stream_mode = cfg->reserved[1];
    // the product form belongs to the handle: fixed here, carried to every launch in the kernels' parameter blocks.  0 resolves
    // to the library default, which the test-only FM_MFMA_SPLIT overrides (read once, here)
    e->products = cfg->reserved[2] == 1 ? 0 : (cfg->reserved[2] == 2 ? 9 : (cfg->reserved[2] == 3 ? 6 : fm_mfma_split()));
    // planes mode: ResNet-18 in a split product form (FM_PLANES=0 keeps the fp32-operand kernels of igemm.hip: the A/B arm)
    e->planes = cfg->model == 0 && cfg->reserved[0] == 0 && e->products != 0 && !(getenv("FM_PLANES") && atoi(getenv("FM_PLANES")) == 0);
    e->dt = e->precision ? DT_BF16 : DT_F32;
    e->fuse_gate = e->precision && !(getenv("FM_FUSE_GATE") && atoi(getenv("FM_FUSE_GATE")) == 0);
    e->cfg = *cfg;
    e->main.st = reinterpret_cast<hipStream_t>(cfg->stream);      // the one assignment of the engine's stream
    e->C = cfg->n_classes; e->H = cfg->in_h; e->W = cfg->in_w; e->maxB = cfg->max_images;
    e->model = cfg->model;
    int rc = e->model == 1 ? build_effnet_b0(e) : build_resnet18(e);
    if (rc == FM_OK) rc = build_tables(e);
    if (rc == FM_OK) rc = build_arena_table(e);
    if (rc == FM_OK) rc = alloc_workspaces(e);
    if (rc != FM_OK) { fm_destroy(e); return rc; }
    *out = e;
    return FM_OK;
}

int fm_destroy(fm_engine* e)
{
    if (!e) return FM_OK;
    (void)hipStreamSynchronize(e->main.st);
    if (e->side.st) { (void)hipStreamSynchronize(e->side.st); (void)hipStreamDestroy(e->side.st); }
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_t) (void)hipEventDestroy(e->ev_t);
    for (int k = 0; k < 4; ++k)
        for (int q = 0; q < 2; ++q) {
            if (e->ev_p[k][q]) (void)hipEventDestroy(e->ev_p[k][q]);
            if (e->ev_c[k][q]) (void)hipEventDestroy(e->ev_c[k][q]);
        }
    if (e->ev_wdone) (void)hipEventDestroy(e->ev_wdone);
    if (e->comm) { (void)fmcomm_destroy(e->comm); e->comm = nullptr; }
    if (e->host_err) (void)hipHostFree(e->host_err);
    for (void* p : e->allocs) (void)hipFree(p);
    for (auto& p : e->evs) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto v : e->ev_free) (void)hipEventDestroy(v);
    delete e;
    return FM_OK;
}

int fm_sync(fm_engine* e)
{
    ARGCHK(e, "null engine");
    HIPCHK(hipStreamSynchronize(e->main.st));
    STEP_DONE(e);
    return FM_OK;
}

int fm_state_sizes(fm_engine* e, int64_t* n_f32, int64_t* n_i64)
{
    ARGCHK(e, "null engine");
    if (n_f32) *n_f32 = e->nf_sd;
    if (n_i64) *n_i64 = e->ni_sd;
    return FM_OK;
}

int fm_set_state(fm_engine* e, const float* host_f32, const int64_t* host_i64)
{
    ARGCHK(e && host_f32, "null engine/state");
    HIPCHK(hipMemcpyAsync(e->stage_sd, host_f32, (size_t)e->nf_sd * 4, hipMemcpyHostToDevice, e->main.st));
    RCCHK(state_dict_to_arena(e, e->stage_sd, e->student.state, false));
    int ic = 0;
    for (auto& en : e->entries)
        if (en.kind == 2) {
            e->student.counters[en.bn] = host_i64 ? host_i64[ic] : 0;
            ++ic;
        }
    HIPCHK(hipStreamSynchronize(e->main.st));
    net_changed(e, e->student);
    return FM_OK;
}

int fm_get_state(fm_engine* e, float* host_f32, int64_t* host_i64)
{
    ARGCHK(e && host_f32, "null engine/state");
    RCCHK(arena_to_state_dict(e, e->student.state, e->stage_sd, false));
    if (host_i64) RCCHK(fm_counters(e, host_i64, 0));
    HIPCHK(hipMemcpyAsync(host_f32, e->stage_sd, (size_t)e->nf_sd * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    return FM_OK;
}

int fm_state_device(fm_engine* e, float** dev_ptr, int64_t* numel)
{
    ARGCHK(e && dev_ptr && numel, "null");
    *dev_ptr = e->student.state;
    *numel = (int64_t)e->NS;
    net_changed(e, e->student);       // the caller is about to overwrite it (all-reduce)
    return FM_OK;
}

int fm_counters(fm_engine* e, int64_t* host_i64, int32_t set)
{
    ARGCHK(e && host_i64, "null");
    int ic = 0;
    for (auto& en : e->entries)
        if (en.kind == 2) {
            if (set) e->student.counters[en.bn] = host_i64[ic];
            else host_i64[ic] = e->student.counters[en.bn];
            ++ic;
        }
    return FM_OK;
}

int fm_state_scale(fm_engine* e, float w)
{
    ARGCHK(e, "null engine");
    k_scale(e->student.state, w, (int64_t)e->NS, e->main.st);
    net_changed(e, e->student);
    return FM_OK;
}

int fm_stream_mode(fm_engine* e)
{
    if (!e) return -1;
    return e->side_ok ? (e->side_w ? 0 : 2) : 1;
}

int fm_mfma_products(void) { return fm_mfma_split(); }
int fm_products(fm_engine* e) { return e ? e->products : FM_ERR_ARG; }
int fm_planes_mode(fm_engine* e) { return e ? (e->planes ? 1 : 0) : FM_ERR_ARG; }

int fm_fedavg_fold(fm_engine* e, const float* const* states_dev, const float* n_host, int32_t K, float* out_dev)
{
    ARGCHK(e && states_dev && n_host && out_dev, "null argument");
    ARGCHK(K >= 1 && K <= FM_FOLD_MAX, "fm_fedavg_fold: 1 <= K <= FM_FOLD_MAX");
    FoldArgs a{};
    float tot = 0.f;                                    // sum(dict_len) as the reference's Python int sum, exact below 2^24
    double tot_d = 0.0;
    for (int k = 0; k < K; ++k) {
        ARGCHK(states_dev[k], "fm_fedavg_fold: null state pointer");
        a.s[k] = states_dev[k];
        a.n[k] = n_host[k];
        tot_d += (double)n_host[k];
    }
    tot = (float)tot_d;
    return fold_states(e, a, K, tot, out_dev);
}

int fm_fed_w(fm_engine* e, const float* const* states_dev, const double* w_host, int32_t K, float* out_dev)
{
    ARGCHK(e && states_dev && w_host && out_dev, "null argument");
    ARGCHK(K >= 1 && K <= FM_FOLD_MAX, "fm_fed_w: 1 <= K <= FM_FOLD_MAX");
    FoldArgs a{};
    double tot_d = 0.0;                                 // Python's sum(weight): in double, rounded to fp32 once
    for (int k = 0; k < K; ++k) {
        ARGCHK(states_dev[k], "fm_fed_w: null state pointer");
        a.s[k] = states_dev[k];
        a.n[k] = (float)w_host[k];
        tot_d += w_host[k];
    }
    return fold_states(e, a, K, (float)tot_d, out_dev);
}

int fm_state_dist(fm_engine* e, const float* const* states_dev, int32_t K, const float* ref_dev, float* norms_dev, int32_t n_entries)
{
    ARGCHK(e && states_dev && norms_dev, "null argument");
    ARGCHK(K >= 1 && K <= FM_FOLD_MAX, "fm_state_dist: 1 <= K <= FM_FOLD_MAX");
    ARGCHK(n_entries == (int32_t)e->tab.ent.size(), "fm_state_dist: n_entries is not the engine's number of fp32 state_dict entries");
    FoldArgs a{};
    for (int k = 0; k < K; ++k) {
        ARGCHK(states_dev[k], "fm_state_dist: null state pointer");
        a.s[k] = states_dev[k];
    }
    if (!e->dist_part) DALLOC(e->dist_part, e->tab.chunks.size() * FM_FOLD_MAX);
    k_state_dist(a, K, ref_dev, e->tab.d_ent, (int)e->tab.ent.size(), e->tab.d_chunks, (int)e->tab.chunks.size(), (int64_t)e->NS,
                 e->dist_part, norms_dev, e->main.st);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

/* ---- RCCL inside the library ------------------------------------------------------------- */
#define COMMCHK(x)                                       \
    do {                                                 \
        if (!(x)) { g_err = fmcomm_error(); return FM_ERR_HIP; } \
    } while (0)

int fm_comm_preflight(void)
{
    COMMCHK(fmcomm_preflight());
    return FM_OK;
}

int fm_comm_unique_id(uint8_t* id128)
{
    ARGCHK(id128, "null id");
    COMMCHK(fmcomm_unique_id(id128));
    return FM_OK;
}

int fm_comm_init(fm_engine* e, const uint8_t* id128, int32_t rank, int32_t world)
{
    ARGCHK(e && id128 && world >= 1 && rank >= 0 && rank < world, "comm arguments");
    if (e->comm) { COMMCHK(fmcomm_destroy(e->comm)); e->comm = nullptr; }
    COMMCHK(fmcomm_init(&e->comm, id128, rank, world));
    e->comm_rank = rank; e->comm_world = world;
    const size_t need = std::max<size_t>((size_t)2 * e->C * e->D + 2 * e->C, e->student.counters.size()) + 64;
    if (e->comm_buf_n < need) { DALLOC(e->comm_buf, need); e->comm_buf_n = need; }
    return FM_OK;
}

int fm_comm_destroy(fm_engine* e)
{
    ARGCHK(e, "null engine");
    if (e->comm) { HIPCHK(hipStreamSynchronize(e->main.st)); COMMCHK(fmcomm_destroy(e->comm)); }
    e->comm = nullptr; e->comm_world = 0;
    return FM_OK;
}

int fm_comm_size(fm_engine* e) { return (e && e->comm) ? e->comm_world : 0; }

int fm_fedavg_allreduce(fm_engine* e, float w)
{
    ARGCHK(e, "null engine");
    k_scale(e->student.state, w, (int64_t)e->NS, e->main.st);
    net_changed(e, e->student);
    if (!e->comm) return FM_OK;      // no communicator: a single client, FedAvg of one = w * state
    // (1) the whole fp32 arena, in place, on the engine stream: the next round's first kernels queue behind it
    COMMCHK(fmcomm_allreduce_sum(e->comm, e->student.state, e->NS, false, e->main.st));
    // (2) num_batches_tracked: weighted mean in float64, truncated on load like utils/FedAvg.py:13 + load_state_dict
    const size_t nb = e->student.counters.size();
    std::vector<double> h(nb);
    for (size_t i = 0; i < nb; ++i) h[i] = (double)w * (double)e->student.counters[i];
    HIPCHK(hipMemcpyAsync(e->comm_buf, h.data(), nb * 8, hipMemcpyHostToDevice, e->main.st));
    COMMCHK(fmcomm_allreduce_sum(e->comm, e->comm_buf, nb, true, e->main.st));
    HIPCHK(hipMemcpyAsync(h.data(), e->comm_buf, nb * 8, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    for (size_t i = 0; i < nb; ++i) e->student.counters[i] = (int64_t)trunc(h[i] + 1e-9);
    return FM_OK;
}

int fm_fedavg_tao(fm_engine* e, const double* t_host, double n_i, const float* negative_mask_host, double* out_host)
{
    ARGCHK(e && t_host && negative_mask_host && out_host, "null");
    const int C = e->C;
    std::vector<double> h(2 * C);
    for (int c = 0; c < C; ++c) {
        const double m = (double)negative_mask_host[c];      // 0/1 for one client; a weight when a rank folds several
        h[c] = m != 0.0 ? t_host[c] * n_i * m : 0.0;
        h[C + c] = n_i * m;
    }
    if (e->comm) {
        HIPCHK(hipMemcpyAsync(e->comm_buf, h.data(), h.size() * 8, hipMemcpyHostToDevice, e->main.st));
        COMMCHK(fmcomm_allreduce_sum(e->comm, e->comm_buf, h.size(), true, e->main.st));
        HIPCHK(hipMemcpyAsync(h.data(), e->comm_buf, h.size() * 8, hipMemcpyDeviceToHost, e->main.st));
        HIPCHK(hipStreamSynchronize(e->main.st));
    }
    for (int c = 0; c < C; ++c) out_host[c] = h[C + c] == 0.0 ? 1.0 : h[c] / h[C + c];   // no active client: 1.0 (:66-67)
    return FM_OK;
}

int fm_fedavg_proto(fm_engine* e, const float* proto_host, double n_i, const float* active_mask_host, float* out_host)
{
    ARGCHK(e && proto_host && active_mask_host && out_host, "null");
    const int C = e->C, D = e->D;
    const size_t np = (size_t)2 * C * D;
    std::vector<float> h(np + 2 * C);
    for (int r = 0; r < 2 * C; ++r) {
        const float wr = (float)(n_i * (double)active_mask_host[r / 2]);   // mask 0/1, or a per-class weight
        for (int d = 0; d < D; ++d) h[(size_t)r * D + d] = wr != 0.f ? proto_host[(size_t)r * D + d] * wr : 0.f;
        h[np + r] = wr;
    }
    if (e->comm) {
        float* buf = reinterpret_cast<float*>(e->comm_buf);
        HIPCHK(hipMemcpyAsync(buf, h.data(), h.size() * 4, hipMemcpyHostToDevice, e->main.st));
        COMMCHK(fmcomm_allreduce_sum(e->comm, buf, h.size(), false, e->main.st));
        HIPCHK(hipMemcpyAsync(h.data(), buf, h.size() * 4, hipMemcpyDeviceToHost, e->main.st));
        HIPCHK(hipStreamSynchronize(e->main.st));
    }
    for (int r = 0; r < 2 * C; ++r)
        for (int d = 0; d < D; ++d) out_host[(size_t)r * D + d] = h[(size_t)r * D + d] / h[np + r];   // 0/0 = NaN row (:85-86)
    return FM_OK;
}

int fm_teacher_snapshot(fm_engine* e)
{
    ARGCHK(e, "null engine");
    HIPCHK(hipMemcpyAsync(e->teacher.state, e->student.state, e->NS * 4, hipMemcpyDeviceToDevice, e->main.st));
    e->teacher.counters = e->student.counters;
    net_changed(e, e->teacher);
    return FM_OK;
}

int fm_adam_reset(fm_engine* e, const fm_adam* hp)
{
    ARGCHK(e, "null engine");
    if (hp) e->hp = *hp;
    return optim_reset(e);
}

int fm_forward_eval(fm_engine* e, const float* x_dev, int32_t B, int32_t use_teacher, float* feat_dev,
                    float* logits_dev)
{
    ARGCHK(e && x_dev, "null");
    ARGCHK(B >= 1 && B <= e->maxB, "B exceeds max_images");
    lane_point(e, 0);
    const float* xs[1] = {x_dev};
    to_nhwc4(e, e->main, xs, 1, B);
    float* feat = use_teacher ? e->tfeat : e->feat;
    float* logits = use_teacher ? e->tlogits : e->logits;
    if (use_teacher) ensure_fwd_shadows(e, e->teacher);
    else ensure_packed(e);
    net_forward_eval(e, e->main, use_teacher ? e->teacher : e->student, e->acts, B, feat, logits);
    if (feat_dev) HIPCHK(hipMemcpyAsync(feat_dev, feat, (size_t)B * e->D * 4, hipMemcpyDeviceToDevice, e->main.st));
    if (logits_dev) HIPCHK(hipMemcpyAsync(logits_dev, logits, (size_t)B * e->C * 4, hipMemcpyDeviceToDevice, e->main.st));
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_step_bce(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B, const float* pos_weight_host,
                int32_t bs_norm, float* loss_dev)
{
    ARGCHK(e && x_dev && y_dev && pos_weight_host && loss_dev, "null");
    return fused_step(e, StepFwd::Student, x_dev, nullptr, B, nullptr, [&] {
        k_loss_bce(e->logits, y_dev, to_cv(pos_weight_host, e->C), B, e->C, 1.f / ((float)bs_norm * (float)e->C), e->dlogits,
                   loss_dev, e->main.st);
    });
}

int fm_step_stage1(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev, int32_t B,
                   const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, float* loss_dev)
{
    ARGCHK(e && x1_dev && x2_dev && y_dev && active_mask_host && loss_dev, "null");
    return fused_step(e, StepFwd::Frozen, x1_dev, x2_dev, B, nullptr, [&] {
        const int n_neg = e->C - count_active(e, active_mask_host);
        k_loss_stage1(e->logits, e->tlogits, y_dev, to_cv(active_mask_host, e->C), B, e->C,
                      1.f / ((float)bs_norm * (float)annotation_num),
                      n_neg ? 1.f / ((float)bs_norm * (float)n_neg) : 0.f, e->dlogits, loss_dev, e->main.st);
    });
}

int fm_step_stage2(fm_engine* e, const float* x_dev, const float* y_dev, const float* distill_dev, int32_t B,
                   float* loss_dev)
{
    ARGCHK(e && x_dev && y_dev && distill_dev && loss_dev, "null");
    return fused_step(e, StepFwd::Student, x_dev, nullptr, B, nullptr,
                      [&] { k_loss_stage2(e->logits, y_dev, distill_dev, B, e->C, e->dlogits, loss_dev, e->main.st); });
}

int fm_step_fixmatch(fm_engine* e, const float* xw_dev, const float* xs_dev, const float* y_dev, int32_t B,
                     const float* pos_weight_host, const float* pos_weight_unk_host, const float* active_mask_host,
                     int32_t annotation_num, int32_t bs_norm, float* loss_dev)
{
    ARGCHK(e && xw_dev && xs_dev && y_dev && pos_weight_host && pos_weight_unk_host && active_mask_host && loss_dev,
           "null");
    // the head's selected-row table holds 2048 rows; past it the batch-size text answers, as it always has
    return fused_step(e, StepFwd::Student, xw_dev, xs_dev, B, B <= 2048 ? nullptr : "2*B exceeds max_images", [&] {
        k_loss_fixmatch(e->logits, y_dev, to_cv(pos_weight_host, e->C), to_cv(pos_weight_unk_host, e->C),
                        to_cv(active_mask_host, e->C), B, e->C, e->C - count_active(e, active_mask_host),
                        1.f / ((float)bs_norm * (float)annotation_num), e->C - annotation_num, e->dlogits, loss_dev, e->main.st);
    });
}

// ---- FedLSR / FedIRM: the heads alone on caller tensors, and the fused FedLSR step ----
int fm_loss_fedlsr(fm_engine* e, const float* z_dev, const float* y_dev, const float* pos_weight_host, float mix1, float beta,
                   int32_t B, float* dz_dev, float* loss_dev)
{
    ARGCHK(e && z_dev && y_dev && pos_weight_host && dz_dev && loss_dev, "null");
    ARGCHK(B >= 1, "B >= 1");
    BADCHK(fedlsr_bad(mix1, false));
    launch_fedlsr(e, z_dev, y_dev, pos_weight_host, mix1, beta, B, dz_dev, loss_dev);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_loss_fedirm_sup(fm_engine* e, const float* z_dev, const float* y_dev, const float* pos_weight_host,
                       const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, int32_t B, float* rel_acc_dev,
                       float* dz_dev, float* loss_dev)
{
    ARGCHK(e && z_dev && y_dev && pos_weight_host && active_mask_host && dz_dev && loss_dev, "null");
    BADCHK(fedirm_bad(B, annotation_num, bs_norm, false));
    k_loss_fedirm_sup(z_dev, y_dev, to_cv(pos_weight_host, e->C), to_cv(active_mask_host, e->C), B, e->C,
                      (float)bs_norm * (float)annotation_num, rel_acc_dev, dz_dev, loss_dev, e->main.st);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_loss_fedirm_rel(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* pos_weight_host,
                       const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, float cw, const float* target_dev,
                       int32_t B, float* rel_acc_dev, float* dz_dev, float* loss_dev)
{
    ARGCHK(e && z_dev && zt_dev && y_dev && pos_weight_host && active_mask_host && target_dev && dz_dev && loss_dev, "null");
    BADCHK(fedirm_bad(B, annotation_num, bs_norm, true));
    k_loss_fedirm_rel(z_dev, zt_dev, y_dev, to_cv(pos_weight_host, e->C), to_cv(active_mask_host, e->C), B, e->C,
                      (float)bs_norm * (float)annotation_num, (float)bs_norm, cw, target_dev, rel_acc_dev, dz_dev,
                      loss_dev, e->main.st);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_step_fedlsr(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev, int32_t B,
                   const float* pos_weight_host, float mix1, float beta, float* loss_dev)
{
    ARGCHK(e && x1_dev && x2_dev && y_dev && pos_weight_host && loss_dev, "null");
    return fused_step(e, StepFwd::Student, x1_dev, x2_dev, B, fedlsr_bad(mix1, true),
                      [&] { launch_fedlsr(e, e->logits, y_dev, pos_weight_host, mix1, beta, B, e->dlogits, loss_dev); });
}

// ---- RSCFed / FedNoRo / CBAFed: the single-view heads on caller tensors, and their fused steps ----
int fm_loss_rscfed(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* pos_weight_host,
                   const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, int32_t B, float* dz_dev, float* loss_dev)
{
    ARGCHK(e && z_dev && zt_dev && y_dev && pos_weight_host && active_mask_host && dz_dev && loss_dev, "null");
    BADCHK(rscfed_bad(e, active_mask_host, annotation_num, bs_norm, B));
    launch_rscfed(e, z_dev, zt_dev, y_dev, pos_weight_host, active_mask_host, annotation_num, bs_norm, B, dz_dev, loss_dev);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_loss_lakd(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* active_mask_host, float w_kd,
                 int32_t B, float* dz_dev, float* loss_dev)
{
    ARGCHK(e && z_dev && zt_dev && y_dev && active_mask_host && dz_dev && loss_dev, "null");
    ARGCHK(B >= 1, "B >= 1");
    BADCHK(classes_bad(e, active_mask_host));
    launch_lakd(e, z_dev, zt_dev, y_dev, active_mask_host, w_kd, B, dz_dev, loss_dev);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_loss_cbafed(fm_engine* e, const float* z_dev, const float* y_dev, const float* active_mask_host, int32_t annotation_num,
                   int32_t bs_norm, const float* tao_host, int32_t B, float* pos_weight_dev, int64_t* counts_dev, float* dz_dev,
                   float* loss_dev)
{
    ARGCHK(e && z_dev && y_dev && active_mask_host && pos_weight_dev && dz_dev && loss_dev, "null");
    BADCHK(cbafed_bad(e, active_mask_host, annotation_num, bs_norm, tao_host, counts_dev, B, false));
    launch_cbafed(e, z_dev, y_dev, active_mask_host, annotation_num, bs_norm, tao_host, B, pos_weight_dev, counts_dev, dz_dev, loss_dev);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

// the skeleton's Rscfed forwards and head, then the teacher's blend with the post-Adam student
int fm_step_rscfed(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev, int32_t B,
                   const float* pos_weight_host, const float* active_mask_host, int32_t annotation_num, int32_t bs_norm,
                   float w_teacher, float w_student, float* loss_dev)
{
    ARGCHK(e && x1_dev && x2_dev && y_dev && pos_weight_host && active_mask_host && loss_dev, "null");
    RCCHK(fused_step(e, StepFwd::Rscfed, x1_dev, x2_dev, B, rscfed_bad(e, active_mask_host, annotation_num, bs_norm, B), [&] {
        launch_rscfed(e, e->logits, e->tlogits, y_dev, pos_weight_host, active_mask_host, annotation_num, bs_norm, B, e->dlogits,
                      loss_dev);
    }));
    RCCHK(fm_teacher_axpby(e, w_teacher, w_student));
    STEP_DONE(e);
    return FM_OK;
}

int fm_step_fednoro(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B, const float* active_mask_host, float w_kd,
                    float* loss_dev)
{
    ARGCHK(e && x_dev && y_dev && active_mask_host && loss_dev, "null");
    return fused_step(e, StepFwd::Frozen, x_dev, nullptr, B, classes_bad(e, active_mask_host),      // both read the one staged view
                      [&] { launch_lakd(e, e->logits, e->tlogits, y_dev, active_mask_host, w_kd, B, e->dlogits, loss_dev); });
}

int fm_step_cbafed(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B, const float* active_mask_host,
                   int32_t annotation_num, int32_t bs_norm, const float* tao_host, float* pos_weight_dev, int64_t* counts_dev,
                   float* loss_dev)
{
    ARGCHK(e && x_dev && y_dev && active_mask_host && pos_weight_dev && loss_dev, "null");
    return fused_step(e, StepFwd::Student, x_dev, nullptr, B,
                      cbafed_bad(e, active_mask_host, annotation_num, bs_norm, tao_host, counts_dev, B, true), [&] {
        launch_cbafed(e, e->logits, y_dev, active_mask_host, annotation_num, bs_norm, tao_host, B, pos_weight_dev, counts_dev,
                      e->dlogits, loss_dev);
    });
}

// ---- RoFL: the head on caller tensors, and its fused step (the head reads the train forward's pooled feature) ----
int fm_loss_rofl(fm_engine* e, const float* z_dev, const float* feat_dev, const float* y_dev, const int32_t* item_dev, int32_t B,
                 int32_t n_keep, const float* pos_weight_host, float lambda_cen_eff, float lambda_e, int32_t write_labels,
                 float* centroids_dev, uint8_t* pseudo_dev, int64_t N, float* dz_dev, float* loss_dev, int32_t* keep_dev)
{
    ARGCHK(e && z_dev && y_dev && pos_weight_host && dz_dev && loss_dev, "null");
    BADCHK(rofl_bad(e, feat_dev, item_dev, centroids_dev, pseudo_dev, B, n_keep, N));
    RCCHK(rofl_ws(e));
    launch_rofl(e, z_dev, feat_dev, y_dev, item_dev, B, n_keep, pos_weight_host, lambda_cen_eff, lambda_e, write_labels,
                centroids_dev, pseudo_dev, N, dz_dev, loss_dev, keep_dev);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_step_rofl(fm_engine* e, const float* x_dev, const float* y_dev, const int32_t* item_dev, int32_t B, int32_t n_keep,
                 const float* pos_weight_host, float lambda_cen_eff, float lambda_e, int32_t write_labels, float* centroids_dev,
                 uint8_t* pseudo_dev, int64_t N, float* loss_dev)
{
    ARGCHK(e && x_dev && y_dev && pos_weight_host && loss_dev, "null");
    const char* bad = rofl_bad(e, e->feat, item_dev, centroids_dev, pseudo_dev, B, n_keep, N);
    if (!bad && e->trainable.empty()) RCCHK(rofl_ws(e));          // a refused call allocates nothing
    return fused_step(e, StepFwd::Student, x_dev, nullptr, B, bad, [&] {
        launch_rofl(e, e->logits, e->feat, y_dev, item_dev, B, n_keep, pos_weight_host, lambda_cen_eff, lambda_e, write_labels,
                    centroids_dev, pseudo_dev, N, e->dlogits, loss_dev, nullptr);
    });
}

int fm_proto_reset(fm_engine* e)
{
    ARGCHK(e, "null engine");
    HIPCHK(hipMemsetAsync(e->psum, 0, (size_t)2 * e->C * e->D * 4, e->main.st));
    HIPCHK(hipMemsetAsync(e->pcnt, 0, (size_t)2 * e->C * 8, e->main.st));
    HIPCHK(hipMemsetAsync(e->tcnt, 0, (size_t)e->C * 8, e->main.st));
    return FM_OK;
}

int fm_proto_accumulate(fm_engine* e, const float* feat_dev, const float* logits_dev, const float* labels_dev,
                        int32_t B, const float* active_mask_host, const float* negative_mask_host, float L, float U)
{
    ARGCHK(e && feat_dev && logits_dev && labels_dev && active_mask_host && negative_mask_host, "null");
    k_proto_accumulate(feat_dev, logits_dev, labels_dev, B, e->D, e->C, to_cv(active_mask_host, e->C),
                       to_cv(negative_mask_host, e->C), L, U, e->psum, e->pcnt, e->tcnt, e->main.st);
    return FM_OK;
}

int fm_proto_finalize(fm_engine* e, int32_t zero_guard, int64_t n_local, const float* active_mask_host,
                      float* proto_host, double* t_host)
{
    ARGCHK(e && active_mask_host && proto_host && t_host, "null");
    std::vector<int64_t> pc(2 * e->C), tc(e->C);
    const int D = e->D;
    HIPCHK(hipMemcpyAsync(proto_host, e->psum, (size_t)2 * e->C * D * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipMemcpyAsync(pc.data(), e->pcnt, pc.size() * 8, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipMemcpyAsync(tc.data(), e->tcnt, tc.size() * 8, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    for (int c = 0; c < e->C; ++c) {
        t_host[c] = (double)tc[c] / (double)n_local;
        if (active_mask_host[c] == 0.f) continue;
        for (int v = 0; v < 2; ++v) {
            const int r = 2 * c + v;
            if (zero_guard && pc[r] == 0) continue;
            const float den = (float)pc[r];
            for (int d = 0; d < D; ++d) proto_host[(size_t)r * D + d] = proto_host[(size_t)r * D + d] / den;
        }
    }
    return FM_OK;
}

int fm_cos_tag(fm_engine* e, const float* feat_dev, int64_t N, const float* proto_dev, const int32_t* classes_host,
               int32_t n_cls, float* sim_dev)
{
    ARGCHK(e && feat_dev && proto_dev && classes_host && sim_dev, "null");
    ARGCHK(n_cls >= 0 && n_cls <= FM_MAX_CLASSES, "n_cls");
    if (n_cls == 0 || N == 0) return FM_OK;
    HIPCHK(hipMemcpyAsync(e->cls_dev, classes_host, (size_t)n_cls * 4, hipMemcpyHostToDevice, e->main.st));
    k_cos_tag(feat_dev, N, e->D, proto_dev, e->cls_dev, n_cls, sim_dev, e->main.st);
    return FM_OK;
}

int fm_select_topk(fm_engine* e, const float* sim_dev, int64_t N, double clean_thr, double noise_thr, int32_t cap,
                   int32_t* top_host, int32_t* n_top, int32_t* bot_host, int32_t* n_bot)
{
    ARGCHK(e && top_host && n_top && bot_host && n_bot, "null");
    *n_top = *n_bot = 0;
    if (N == 0) return FM_OK;              // an empty pool selects nothing (sim_dev may be NULL then)
    ARGCHK(sim_dev, "null sim_dev");
    int counts[2];
    k_count_sign(sim_dev, N, e->sel_counts, e->main.st);
    HIPCHK(hipMemcpyAsync(counts, e->sel_counts, 8, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    const int kt = (int)(1 * clean_thr * counts[0]);      // int() truncation as in :1069-1070
    const int kb = (int)(1 * noise_thr * counts[1]);
    ARGCHK(kt <= cap && kb <= cap, "selection exceeds cap");
    if (kt == 0 && kb == 0) return FM_OK;
    if (e->sel_cap < std::max(kt, kb)) {
        e->sel_cap = std::max(std::max(kt, kb), 1024);
        DALLOC(e->sel_top, e->sel_cap);
        DALLOC(e->sel_bot, e->sel_cap);
    }
    k_rank_select(sim_dev, N, kt, kb, e->sel_top, e->sel_bot, e->main.st);
    if (kt) HIPCHK(hipMemcpyAsync(top_host, e->sel_top, (size_t)kt * 4, hipMemcpyDeviceToHost, e->main.st));
    if (kb) HIPCHK(hipMemcpyAsync(bot_host, e->sel_bot, (size_t)kb * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    *n_top = kt; *n_bot = kb;
    return FM_OK;
}

int fm_select_topk_rows(fm_engine* e, const float* sim_dev, int64_t N, int32_t n_cls, const int32_t* pool_rows_host,
                        const int32_t* pool_n_host, int32_t stride, double clean_thr, double noise_thr, int32_t cap,
                        int32_t* top_host, int32_t* n_top, int32_t* bot_host, int32_t* n_bot)
{
    ARGCHK(e && pool_n_host && top_host && n_top && bot_host && n_bot, "null");
    ARGCHK(n_cls >= 0 && n_cls <= FM_MAX_CLASSES && cap >= 1, "n_cls / cap");
    for (int k = 0; k < n_cls; ++k) n_top[k] = n_bot[k] = 0;
    if (n_cls == 0 || N == 0) return FM_OK;
    ARGCHK(sim_dev, "null sim_dev");
    int maxn = 0;
    for (int k = 0; k < n_cls; ++k) {
        ARGCHK(pool_n_host[k] >= 0 && pool_n_host[k] <= (pool_rows_host ? stride : N), "pool size");
        maxn = std::max(maxn, pool_n_host[k]);
        // a row outside [0, N) would be an out-of-bounds read of sim in the counting / ranking kernels
        if (pool_rows_host)
            for (int i = 0; i < pool_n_host[k]; ++i) {
                const int32_t r = pool_rows_host[(size_t)k * stride + i];
                ARGCHK(r >= 0 && (int64_t)r < N, "pool row outside [0, N)");
            }
    }
    const size_t rows_ints = pool_rows_host ? (size_t)n_cls * stride : 0;
    const size_t need = (size_t)n_cls * (3 + 2 * (size_t)cap) + rows_ints;
    if (e->tag_buf_ints < need) {
        if (e->tag_buf) {               // the outgrown buffer goes back now, not at fm_destroy (the stream may still read it)
            HIPCHK(hipStreamSynchronize(e->main.st));
            auto it = std::find(e->allocs.begin(), e->allocs.end(), (void*)e->tag_buf);
            if (it != e->allocs.end()) e->allocs.erase(it);
            (void)hipFree(e->tag_buf);
            e->tag_buf = nullptr; e->tag_buf_ints = 0;
        }
        const size_t want = need + need / 2;
        DALLOC(e->tag_buf, want);
        e->tag_buf_ints = want;
    }
    int* d_pn = e->tag_buf;
    int* d_counts = d_pn + n_cls;
    int* d_top = d_counts + 2 * n_cls;
    int* d_bot = d_top + (size_t)n_cls * cap;
    int* d_rows = pool_rows_host ? d_bot + (size_t)n_cls * cap : nullptr;
    HIPCHK(hipMemcpyAsync(d_pn, pool_n_host, (size_t)n_cls * 4, hipMemcpyHostToDevice, e->main.st));
    if (d_rows) HIPCHK(hipMemcpyAsync(d_rows, pool_rows_host, rows_ints * 4, hipMemcpyHostToDevice, e->main.st));
    k_select_rows(sim_dev, N, n_cls, d_rows, d_pn, stride, maxn, clean_thr, noise_thr, cap, d_counts, d_top, d_bot, e->main.st);
    // ONE device-to-host read: the counts and both pick tables
    std::vector<int> h((size_t)n_cls * (2 + 2 * (size_t)cap));
    HIPCHK(hipMemcpyAsync(h.data(), d_counts, h.size() * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    for (int k = 0; k < n_cls; ++k) {
        const int kt = (int)(1 * clean_thr * h[2 * k]), kb = (int)(1 * noise_thr * h[2 * k + 1]);     // int() truncation as in :1069-1070
        ARGCHK(kt <= cap && kb <= cap, "selection exceeds cap");
        n_top[k] = kt; n_bot[k] = kb;
        memcpy(top_host + (size_t)k * cap, h.data() + 2 * n_cls + (size_t)k * cap, (size_t)kt * 4);
        memcpy(bot_host + (size_t)k * cap, h.data() + 2 * n_cls + (size_t)n_cls * cap + (size_t)k * cap, (size_t)kb * 4);
    }
    return FM_OK;
}

int fm_augment(fm_engine* e, const uint8_t* cache_dev, const int32_t* idx_dev, const int32_t* params_dev, int32_t B,
               const float* mean_host, const float* std_host, float* out_dev)
{
    ARGCHK(e && cache_dev && idx_dev && params_dev && mean_host && std_host && out_dev && B >= 1, "null");
    k_augment(cache_dev, idx_dev, params_dev, out_dev, B, e->H, e->W, mean_host[0], mean_host[1], mean_host[2],
              std_host[0], std_host[1], std_host[2], e->main.st);
    return FM_OK;
}

int fm_augment_strong(fm_engine* e, const uint8_t* cache_dev, const int32_t* idx_dev, const int32_t* params_dev,
                      const int32_t* strong_dev, int32_t B, const float* mean_host, const float* std_host, float* out_dev)
{
    ARGCHK(e && cache_dev && idx_dev && params_dev && strong_dev && mean_host && std_host && out_dev, "null");
    ARGCHK(B >= 1 && B <= e->maxB, "B exceeds max_images");
    ARGCHK(e->W % 4 == 0 && e->H >= 1, "the strong view packs four pixels of a row per thread: W % 4 == 0");
    if (!e->strong_ws) DALLOC(e->strong_ws, fm_strong_ws_bytes(e->maxB, e->H, e->W));    // first use: weak-only users never pay for it
    k_augment_strong(cache_dev, idx_dev, params_dev, strong_dev, e->strong_ws, e->maxB, out_dev, B, e->H, e->W, mean_host[0],
                     mean_host[1], mean_host[2], std_host[0], std_host[1], std_host[2], e->main.st);
    return FM_OK;
}

int fm_eval_metrics(fm_engine* e, const float* scores_dev, const float* labels_dev, int64_t N, int32_t C, float threshold,
                    double* ap_dev, double* auc_dev, int64_t* counts_dev)
{
    ARGCHK(e && scores_dev && labels_dev, "null argument");
    ARGCHK(C >= 1 && C <= FM_MAX_CLASSES, "fm_eval_metrics: 1 <= C <= FM_MAX_CLASSES");
    ARGCHK(N >= 1 && N <= ((int64_t)1 << 22), "fm_eval_metrics: 1 <= N <= 2^22");
    if (!ap_dev && !auc_dev && !counts_dev) return FM_OK;
    const size_t need = fm_metrics_ws_bytes(N, C);
    if (e->metrics_ws_bytes < need) {
        if (e->metrics_ws) {            // the outgrown workspace goes back now (the stream may still read it)
            HIPCHK(hipStreamSynchronize(e->main.st));
            auto it = std::find(e->allocs.begin(), e->allocs.end(), (void*)e->metrics_ws);
            if (it != e->allocs.end()) e->allocs.erase(it);
            (void)hipFree(e->metrics_ws);
            e->metrics_ws = nullptr; e->metrics_ws_bytes = 0;
        }
        DALLOC(e->metrics_ws, need);
        e->metrics_ws_bytes = need;
    }
    k_eval_metrics(scores_dev, labels_dev, N, C, threshold, e->metrics_ws, ap_dev, auc_dev, counts_dev, e->main.st);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_forward_train(fm_engine* e, const float* x1_dev, const float* x2_dev, int32_t B, float* feat_dev,
                     float* logits_dev)
{
    ARGCHK(e && x1_dev, "null");
    const int views = x2_dev ? 2 : 1;
    ARGCHK(B >= 1 && views * B <= e->maxB, "views*B exceeds max_images");
    lane_point(e, 0);
    const float* xs[2] = {x1_dev, x2_dev};
    to_nhwc4(e, e->main, xs, views, B);
    net_forward_train(e, views, B, e->bn_freeze ? BnMode::Frozen : BnMode::Batch);
    if (feat_dev)
        HIPCHK(hipMemcpyAsync(feat_dev, e->feat, (size_t)views * B * e->D * 4, hipMemcpyDeviceToDevice, e->main.st));
    if (logits_dev)
        HIPCHK(hipMemcpyAsync(logits_dev, e->logits, (size_t)views * B * e->C * 4, hipMemcpyDeviceToDevice, e->main.st));
    e->pending_views = views; e->pending_B = B; e->pending_fixed = e->bn_freeze;
    e->pending_trainable = e->trainable;
    STEP_DONE(e);
    return FM_OK;
}

int fm_bn_freeze(fm_engine* e, int32_t on)
{
    ARGCHK(e, "null engine");
    e->bn_freeze = on != 0;
    return FM_OK;
}

int fm_bn_frozen(fm_engine* e)
{
    return e && e->bn_freeze ? 1 : 0;
}

int fm_backward_step(fm_engine* e, const float* dlogits_dev)
{
    ARGCHK(e && dlogits_dev, "null");
    ARGCHK(e->pending_views > 0, "fm_backward_step without a preceding fm_forward_train");
    ARGCHK(e->trainable.empty() && e->pending_trainable.empty(), kMaskRefusal);      // the current mask and the pending forward's
    const int views = e->pending_views, B = e->pending_B;
    lane_point(e, 0);
    HIPCHK(hipMemcpyAsync(e->dlogits, dlogits_dev, (size_t)views * B * e->C * 4, hipMemcpyDeviceToDevice, e->main.st));
    Bwd bw;
    bw.frozen = e->pending_fixed;
    net_backward_and_step(e, views, B, bw);
    e->pending_views = 0;
    STEP_DONE(e);
    return FM_OK;
}

int fm_backward_grads(fm_engine* e, const float* dlogits_dev, const float* dfeat_dev)
{
    return fm_backward_grads_x(e, dlogits_dev, dfeat_dev, nullptr, nullptr);
}

int fm_backward_grads_x(fm_engine* e, const float* dlogits_dev, const float* dfeat_dev, float* dx1_dev, float* dx2_dev)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->pending_views > 0, "fm_backward_grads(_x) without a preceding fm_forward_train / fm_forward_recompute");
    const int views = e->pending_views, B = e->pending_B;
    ARGCHK(views == 2 || !dx2_dev, "fm_backward_grads_x: dx2 given, but the pending forward has one view");
    lane_point(e, 0);
    if (dx1_dev || dx2_dev) {                      // first use: the stem's weights as the data gradient's B matrix
        RCCHK(ensure_stem_dpack(e));
    }
    if (!e->gacc) {                                // first use: fused-only users never pay for the accumulator
        DALLOC(e->gacc, e->NP);
        HIPCHK(hipMemsetAsync(e->gacc, 0, e->NP * 4, e->main.st));     // zeroed at allocation like every arena (padding)
    }
    const size_t nz = (size_t)views * B * e->C * 4;
    if (dlogits_dev) HIPCHK(hipMemcpyAsync(e->dlogits, dlogits_dev, nz, hipMemcpyDeviceToDevice, e->main.st));
    else HIPCHK(hipMemsetAsync(e->dlogits, 0, nz, e->main.st));
    Bwd bw;
    bw.frozen = e->pending_fixed; bw.dfeat = dfeat_dev; bw.dx[0] = dx1_dev; bw.dx[1] = dx2_dev; bw.step = false;
    // the mask the pending forward ran under (empty = every parameter: the flat pass, as ever)
    const bool masked = !e->pending_trainable.empty();
    if (masked) bw.train = e->pending_trainable.data();
    net_backward_and_step(e, views, B, bw);      // e->grad, every weight gradient joined to the main lane
    // Masking happens IN the copy / accumulate pass: its table-driven form copies or adds the trainable entries' spans, writes
    // zeros over the frozen ones (stale in e->grad where a launch was skipped) and touches nothing outside the entries (zero
    // since the accumulator was allocated)
    if (!masked) k_grad_accumulate(e->gacc, e->grad, (int64_t)e->NP, !e->gacc_full, e->main.st, e->dev_err);
    else k_grad_accumulate_masked(e->gacc, e->grad, e->tab.d_chunks, e->tab.n_param_chunks, mask_sel(e, bw.train), !e->gacc_full, e->main.st,
                                  e->dev_err);
    e->pending_views = 0;
    STEP_DONE(e);
    e->gacc_full = true;
    return FM_OK;
}

int fm_forward_recompute(fm_engine* e, const float* x1_dev, const float* x2_dev, int32_t B)
{
    ARGCHK(e && x1_dev, "null");
    const int views = x2_dev ? 2 : 1;
    ARGCHK(B >= 1 && views * B <= e->maxB, "views*B exceeds max_images");
    lane_point(e, 0);
    const float* xs[2] = {x1_dev, x2_dev};
    to_nhwc4(e, e->main, xs, views, B);
    net_forward_train(e, views, B, e->bn_freeze ? BnMode::Frozen : BnMode::BatchNoUpdate);
    e->pending_views = views; e->pending_B = B; e->pending_fixed = e->bn_freeze;
    e->pending_trainable = e->trainable;
    STEP_DONE(e);
    return FM_OK;
}

int fm_zero_grad(fm_engine* e)
{
    ARGCHK(e, "null engine");
    e->gacc_full = false;
    return FM_OK;
}

int fm_adam_step(fm_engine* e, const fm_adam* hp)
{
    ARGCHK(e && hp, "null");
    e->hp = *hp;
    if (!e->gacc_full) return FM_OK;               // torch.optim.Adam skips parameters whose .grad is None
    adam_step(e, e->gacc);
    STEP_DONE(e);
    return FM_OK;
}

int fm_get_grads(fm_engine* e, float* dev_out)
{
    ARGCHK(e && dev_out, "null");
    if (!e->gacc_full) HIPCHK(hipMemsetAsync(dev_out, 0, (size_t)e->nf_sd * 4, e->main.st));
    else {
        RCCHK(arena_to_state_dict(e, e->gacc, dev_out, true));
    }
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_sgd_reset(fm_engine* e, const fm_sgd* hp)
{
    ARGCHK(e, "null engine");
    BADCHK(hp ? sgd_bad(hp) : nullptr);
    return optim_reset(e);
}

int fm_sgd_step(fm_engine* e, const fm_sgd* hp)
{
    ARGCHK(e && hp, "null");
    BADCHK(sgd_bad(hp));
    if (!e->gacc_full) return FM_OK;               // torch.optim.SGD skips parameters whose .grad is None
    sgd_step(e, *hp);
    STEP_DONE(e);
    return FM_OK;
}

int fm_adamw_step(fm_engine* e, const fm_adam* hp)
{
    ARGCHK(e && hp, "null");
    BADCHK(adam_bad(hp));
    if (!e->gacc_full) return FM_OK;
    adamw_step(e, *hp);
    STEP_DONE(e);
    return FM_OK;
}

int fm_set_trainable(fm_engine* e, const int32_t* flags, int32_t n_entries)
{
    ARGCHK(e && flags, "null");
    ARGCHK(n_entries == (int32_t)e->entries.size(), "fm_set_trainable: one flag per state entry (fm_state_sizes' entry count)");
    bool all = true;
    for (size_t i = 0; i < e->entries.size(); ++i)
        if (is_param(e, e->entries[i]) && !flags[i]) all = false;
    e->trainable.clear();                          // the default mask is the EMPTY one: nothing then differs from a handle without masks
    if (!all) {
        e->trainable.assign(e->entries.size(), 0);
        for (size_t i = 0; i < e->entries.size(); ++i) e->trainable[i] = is_param(e, e->entries[i]) && flags[i] ? 1 : 0;
    }
    return FM_OK;
}

int fm_get_trainable(fm_engine* e, int32_t* flags, int32_t n_entries)
{
    ARGCHK(e && flags, "null");
    ARGCHK(n_entries == (int32_t)e->entries.size(), "fm_get_trainable: one flag per state entry");
    for (size_t i = 0; i < e->entries.size(); ++i)
        flags[i] = is_param(e, e->entries[i]) && (e->trainable.empty() || e->trainable[i]) ? 1 : 0;
    return FM_OK;
}

int fm_optim_groups(fm_engine* e, const int32_t* group_of_entry, int32_t n_entries, int32_t n_groups)
{
    ARGCHK(e, "null engine");
    ARGCHK(n_groups >= 0 && n_groups <= FM_MAX_GROUPS, "fm_optim_groups: n_groups must be in 0 .. FM_MAX_GROUPS");
    if (n_groups == 0) { e->group_of.clear(); e->n_groups = 0; return FM_OK; }
    ARGCHK(group_of_entry && n_entries == (int32_t)e->entries.size(), "fm_optim_groups: one group per state entry");
    for (size_t i = 0; i < e->entries.size(); ++i)
        ARGCHK(!is_param(e, e->entries[i]) || (group_of_entry[i] >= -1 && group_of_entry[i] < n_groups),
               "fm_optim_groups: a group index outside -1 .. n_groups - 1");
    e->group_of.assign(e->entries.size(), -1);
    for (size_t i = 0; i < e->entries.size(); ++i)
        if (is_param(e, e->entries[i])) e->group_of[i] = group_of_entry[i];
    e->n_groups = n_groups;
    return FM_OK;
}

int fm_adam_step_groups(fm_engine* e, const fm_adam* hp, int32_t n)
{
    ARGCHK(e && hp, "null");
    ARGCHK(n >= 1 && n == e->n_groups, "fm_adam_step_groups: n must be the group count of the installed fm_optim_groups table");
    for (int i = 0; i < n; ++i) BADCHK(adam_bad(&hp[i]));
    if (!e->gacc_full) return FM_OK;
    adam_step_groups(e, hp, n);
    STEP_DONE(e);
    return FM_OK;
}

int fm_adamw_step_groups(fm_engine* e, const fm_adam* hp, int32_t n)
{
    ARGCHK(e && hp, "null");
    ARGCHK(n >= 1 && n == e->n_groups, "fm_adamw_step_groups: n must be the group count of the installed fm_optim_groups table");
    for (int i = 0; i < n; ++i) BADCHK(adam_bad(&hp[i]));
    if (!e->gacc_full) return FM_OK;
    adamw_step_groups(e, hp, n);
    STEP_DONE(e);
    return FM_OK;
}

int fm_sgd_step_groups(fm_engine* e, const fm_sgd* hp, int32_t n)
{
    ARGCHK(e && hp, "null");
    ARGCHK(n >= 1 && n == e->n_groups, "fm_sgd_step_groups: n must be the group count of the installed fm_optim_groups table");
    for (int i = 0; i < n; ++i) BADCHK(sgd_bad(&hp[i]));
    if (!e->gacc_full) return FM_OK;
    sgd_step_groups(e, hp, n);
    STEP_DONE(e);
    return FM_OK;
}

int fm_grad_norm(fm_engine* e, float* norm_dev)
{
    ARGCHK(e && norm_dev, "null");
    if (!e->gacc_full) HIPCHK(hipMemsetAsync(norm_dev, 0, sizeof(float), e->main.st));
    else RCCHK(grad_norm(e, norm_dev));
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_clip_grad_norm(fm_engine* e, float max_norm, float* norm_dev)
{
    ARGCHK(e, "null engine");
    ARGCHK(max_norm >= 0.f, "fm_clip_grad_norm: max_norm must be >= 0");
    if (!e->gacc_full) {
        if (norm_dev) HIPCHK(hipMemsetAsync(norm_dev, 0, sizeof(float), e->main.st));
        return FM_OK;
    }
    RCCHK(grad_norm(e, norm_dev ? norm_dev : e->norm_word));
    k_grad_clip_norm(e->gacc, (int64_t)e->NP, norm_dev ? norm_dev : e->norm_word, max_norm, e->main.st, e->dev_err);
    STEP_DONE(e);
    return FM_OK;
}

int fm_clip_grad_value(fm_engine* e, float clip)
{
    ARGCHK(e, "null engine");
    ARGCHK(clip >= 0.f, "fm_clip_grad_value: clip must be >= 0");
    if (!e->gacc_full) return FM_OK;
    k_grad_clip_value(e->gacc, (int64_t)e->NP, clip, e->main.st, e->dev_err);
    STEP_DONE(e);
    return FM_OK;
}

int fm_optim_get_state(fm_engine* e, float* m_dev, float* v_dev, int64_t* step_host)
{
    ARGCHK(e, "null engine");
    if (m_dev) RCCHK(arena_to_state_dict(e, e->adam_m, m_dev, true));
    if (v_dev) RCCHK(arena_to_state_dict(e, e->adam_v, v_dev, true));
    if (step_host) *step_host = e->adam_t;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_optim_set_state(fm_engine* e, const float* m_dev, const float* v_dev, int64_t step)
{
    ARGCHK(e && m_dev, "null");
    ARGCHK(step >= 0, "fm_optim_set_state: step must be >= 0");
    RCCHK(optim_reset(e));                         // the padding of both arenas is zero from here on
    RCCHK(state_dict_to_arena(e, m_dev, e->adam_m, true));
    if (v_dev) RCCHK(state_dict_to_arena(e, v_dev, e->adam_v, true));
    e->adam_t = step;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

// ---- client-drift correction (include/fedmlp_hip_drift.h) --------------------------------------------------------------
int fm_drift_begin(fm_engine* e, float mu, const float* shift_dev, int32_t track)
{
    ARGCHK(e, "null engine");
    ARGCHK(!e->drift_on, "fm_drift_begin: a correction is already installed (fm_drift_end first)");
    ARGCHK(mu >= 0.f && std::isfinite(mu), "fm_drift_begin: mu must be finite and >= 0");
    ARGCHK(mu != 0.f || shift_dev || track, "fm_drift_begin: nothing to install (mu == 0, no shift, track == 0)");
    // first install: the arenas this one needs, zeroed at allocation like every arena (padding)
    for (float** p : {&e->drift_anchor, &e->drift_gcorr, shift_dev ? &e->drift_shift : nullptr, track ? &e->drift_gsum : nullptr}) {
        if (!p || *p) continue;
        DALLOC(*p, e->NP);
        HIPCHK(hipMemsetAsync(*p, 0, e->NP * 4, e->main.st));
    }
    HIPCHK(hipMemcpyAsync(e->drift_anchor, e->student.state, e->NP * 4, hipMemcpyDeviceToDevice, e->main.st));
    if (shift_dev) {
        HIPCHK(hipMemsetAsync(e->drift_shift, 0, e->NP * 4, e->main.st));      // the padding of the arena is zero from here on
        RCCHK(state_dict_to_arena(e, shift_dev, e->drift_shift, true));
    }
    if (track) HIPCHK(hipMemsetAsync(e->drift_gsum, 0, e->NP * 4, e->main.st));
    e->drift_mu = mu; e->drift_shifted = shift_dev != nullptr; e->drift_track = track != 0;
    e->drift_steps = 0;
    e->drift_on = true;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_drift_last(fm_engine* e, float* out_dev)
{
    ARGCHK(e && out_dev, "null");
    ARGCHK(e->drift_gcorr && e->drift_steps > 0, "fm_drift_last: no optimizer step since fm_drift_begin");
    RCCHK(arena_to_state_dict(e, e->drift_gcorr, out_dev, true));
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_drift_end(fm_engine* e, float* mean_dev, int64_t* steps_host)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->drift_on, "fm_drift_end: no correction is installed");
    if (mean_dev) {
        if (e->drift_track && e->drift_steps > 0) {
            // the division commutes with the change of layout: S in net.grads() order first, then S / (float)K in place
            RCCHK(arena_to_state_dict(e, e->drift_gsum, mean_dev, true));
            k_drift_div(mean_dev, (float)e->drift_steps, e->nf_sd, e->main.st);
        } else {
            HIPCHK(hipMemsetAsync(mean_dev, 0, (size_t)e->nf_sd * 4, e->main.st));
        }
    }
    if (steps_host) *steps_host = e->drift_steps;
    e->drift_on = false;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_drift_active(fm_engine* e) { return e && e->drift_on ? 1 : 0; }

// ---- server optimizers (include/fedmlp_hip_server.h) -------------------------------------------------------------------
namespace {
inline bool srv_adaptive(int rule) { return rule != FM_SERVER_AVGM; }
inline int srv_fill(fm_engine* e, float* p, float value)
{
    uint32_t bits;
    memcpy(&bits, &value, 4);
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)bits, e->NP, e->main.st));
    return FM_OK;
}
}  // namespace

int fm_server_opt_begin(fm_engine* e, const fm_server_opt* hp)
{
    ARGCHK(e && hp, "null");
    ARGCHK(!e->srv_on, "fm_server_opt_begin: a server optimizer is already installed (fm_server_opt_end first)");
    ARGCHK(hp->rule >= FM_SERVER_AVGM && hp->rule <= FM_SERVER_YOGI, "fm_server_opt_begin: unknown rule");
    ARGCHK(hp->lr >= 0.f && std::isfinite(hp->lr), "fm_server_opt_begin: lr must be finite and >= 0");
    ARGCHK(hp->beta1 >= 0.f && hp->beta1 < 1.f, "fm_server_opt_begin: beta1 must lie in [0, 1)");
    const bool second = hp->rule == FM_SERVER_ADAM || hp->rule == FM_SERVER_YOGI;
    ARGCHK(!second || (hp->beta2 >= 0.f && hp->beta2 < 1.f), "fm_server_opt_begin: beta2 must lie in [0, 1)");
    ARGCHK(!srv_adaptive(hp->rule) || (std::isfinite(hp->tau) && hp->tau > 0.f), "fm_server_opt_begin: tau must be finite and > 0");
    if (!e->srv_part) DALLOC(e->srv_part, (size_t)e->tab.n_param_chunks);
    if (!e->srv_m) DALLOC(e->srv_m, e->NP);
    if (srv_adaptive(hp->rule) && !e->srv_v) DALLOC(e->srv_v, e->NP);
    HIPCHK(hipMemsetAsync(e->srv_m, 0, e->NP * 4, e->main.st));
    if (srv_adaptive(hp->rule)) {
#pragma clang fp contract(off)
        const float v0 = hp->tau * hp->tau;
        RCCHK(srv_fill(e, e->srv_v, v0));
    }
    e->srv_hp = *hp;
    e->srv_omb1 = 1.0f - hp->beta1; e->srv_omb2 = 1.0f - hp->beta2;
    e->srv_steps = 0;
    e->srv_on = true;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_server_opt_step(fm_engine* e, const float* x_old_dev, double* delta_norm_dev)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->srv_on, "fm_server_opt_step: no server optimizer is installed");
    ARGCHK(x_old_dev, "fm_server_opt_step: null x_old_dev");
    ARGCHK(x_old_dev + e->NS <= e->student.state || x_old_dev >= e->student.state + e->NS,
           "fm_server_opt_step: x_old_dev is the engine's own state buffer");
    // the state as a writer gets it: fm_state_device raises every staleness flag fm_state_scale and fm_fedavg_allreduce raise
    float* st = nullptr;
    int64_t ns = 0;
    RCCHK(fm_state_device(e, &st, &ns));
    OP(e->main, "server_opt");
    const fm_server_opt& hp = e->srv_hp;
    const ServerOps a{x_old_dev, st, e->srv_m, e->srv_v, hp.lr, hp.beta1, e->srv_omb1, hp.beta2, e->srv_omb2, hp.tau};
    k_server_opt(hp.rule, a, e->tab.d_ent, e->tab.d_chunks, e->tab.n_param_chunks, e->srv_part, delta_norm_dev, e->main.st, e->dev_err);
    e->srv_steps += 1;
    STEP_DONE(e);
    return FM_OK;
}

int fm_server_opt_get_state(fm_engine* e, float* m_dev, float* v_dev, int64_t* steps_host)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->srv_on, "fm_server_opt_get_state: no server optimizer is installed");
    if (m_dev) RCCHK(arena_to_state_dict(e, e->srv_m, m_dev, true));
    if (v_dev) {
        if (srv_adaptive(e->srv_hp.rule)) RCCHK(arena_to_state_dict(e, e->srv_v, v_dev, true));
        else HIPCHK(hipMemsetAsync(v_dev, 0, (size_t)e->nf_sd * 4, e->main.st));
    }
    if (steps_host) *steps_host = e->srv_steps;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_server_opt_set_state(fm_engine* e, const float* m_dev, const float* v_dev, int64_t steps)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->srv_on, "fm_server_opt_set_state: no server optimizer is installed");
    const bool adaptive = srv_adaptive(e->srv_hp.rule);
    ARGCHK(m_dev && (v_dev || !adaptive), "fm_server_opt_set_state: null moment");
    ARGCHK(steps >= 0, "fm_server_opt_set_state: steps must be >= 0");
    // the floats outside the entries' matrices keep a legal value: m = 0, v = tau^2 as at the install
    HIPCHK(hipMemsetAsync(e->srv_m, 0, e->NP * 4, e->main.st));
    RCCHK(state_dict_to_arena(e, m_dev, e->srv_m, true));
    if (adaptive) {
#pragma clang fp contract(off)
        const float v0 = e->srv_hp.tau * e->srv_hp.tau;
        RCCHK(srv_fill(e, e->srv_v, v0));
        RCCHK(state_dict_to_arena(e, v_dev, e->srv_v, true));
    }
    e->srv_steps = steps;
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_server_opt_end(fm_engine* e)
{
    ARGCHK(e, "null engine");
    ARGCHK(e->srv_on, "fm_server_opt_end: no server optimizer is installed");
    e->srv_on = false;
    return FM_OK;
}

int fm_server_opt_active(fm_engine* e) { return e && e->srv_on ? 1 : 0; }

int fm_teacher_axpby(fm_engine* e, float w_teacher, float w_student)
{
    ARGCHK(e, "null engine");
    k_axpby(e->teacher.state, e->student.state, w_teacher, w_student, (int64_t)e->NS, e->main.st);
    // int64 num_batches_tracked: the float result is truncated when it is loaded back (like FedAvg, Q7)
    for (size_t i = 0; i < e->student.counters.size(); ++i)
        e->teacher.counters[i] = (int64_t)(w_teacher * (float)e->teacher.counters[i] + w_student * (float)e->student.counters[i]);
    net_changed(e, e->teacher);
    return FM_OK;
}

int fm_teacher_ema_params(fm_engine* e, double alpha)
{
    ARGCHK(e, "null engine");
    ARGCHK(alpha >= 0.0 && alpha <= 1.0, "fm_teacher_ema_params: alpha in [0, 1]");
    // the trainable part of the arena only: running statistics (behind NP) and the counters stay as they are
    k_axpby(e->teacher.state, e->student.state, (float)alpha, (float)(1.0 - alpha), (int64_t)e->NP, e->main.st);
    net_changed(e, e->teacher);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_teacher_swap(fm_engine* e)
{
    ARGCHK(e, "null engine");
    std::swap(e->student, e->teacher);        // each net's affine and forward shadows go along, and so do their flags
    student_copies_stale(e);
    return FM_OK;
}

int fm_set_stochastic(fm_engine* e, const float* drop_connect_dev, const float* dropout_dev)
{
    ARGCHK(e, "null engine");
    e->dc_dev = drop_connect_dev;
    e->drop_dev = dropout_dev;
    return FM_OK;
}

int fm_feature_dim(fm_engine* e) { return e ? e->D : 0; }

int fm_profile_enable(fm_engine* e, int32_t on)
{
    ARGCHK(e, "null engine");
    e->prof = on != 0;
    return FM_OK;
}

int fm_profile_read(fm_engine* e, int32_t family, int64_t* launches, double* ms, double* flops)
{
    ARGCHK(e && family >= 0 && family < FM_PROFILE_FAMILIES, "family");
    HIPCHK(hipStreamSynchronize(e->main.st));
    if (e->prof_fail) { e->prof_fail = false; g_err = "a profiling event could not be created/recorded"; return FM_ERR_HIP; }
    for (auto& p : e->evs) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
            e->prof_ms[p.family] += t; e->prof_flops[p.family] += p.flops; e->prof_n[p.family] += 1;
        }
        e->ev_free.push_back(p.a); e->ev_free.push_back(p.b);
    }
    e->evs.clear();
    if (launches) *launches = e->prof_n[family];
    if (ms) *ms = e->prof_ms[family];
    if (flops) *flops = e->prof_flops[family];
    e->prof_n[family] = 0; e->prof_ms[family] = 0; e->prof_flops[family] = 0;
    return FM_OK;
}

// the bf16 stem's operand, as to_nhwc4 forms it: the im2col matrix of `groups` views of imgs / groups images of the fp32 NCHW batch x
static void debug_stem_col(fm_engine* e, const Conv& c, const float* x, int imgs, int groups)
{
    const int B = imgs / groups;
    for (int g = 0; g < groups; ++g)
        k_stem_im2col(x + (size_t)g * B * 3 * e->H * e->W, reinterpret_cast<bf16*>(e->stem_col) + (size_t)g * B * c.hout * c.wout * c.Kw, B,
                      e->H, e->W, c.hout, c.wout, c.k, c.stride, c.pad, c.pad, e->main.st);
}

int fm_debug_pw(fm_engine* e, int32_t op, int32_t conv, const void* x_dev, const void* dy_dev, void* out_dev,
                int32_t imgs, int32_t groups, const float* psc_dev, const float* psh_dev, const float* gate_dev,
                float* stats_dev)
{
    ARGCHK(e && out_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    const bool stem = e->precision == 1 && e->model == 1 && e->convs[conv].cin == 3 && op == 2;    // the stem's weight gradient only
    ARGCHK(e->precision == 1 && (e->convs[conv].k == 1 || stem), "bf16 engine and a 1x1 convolution");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs/groups");
    Conv& c = e->convs[conv];
    ARGCHK(!stem || (x_dev && !gate_dev && !psc_dev && !psh_dev), "the stem takes its NCHW batch and no prologue");
    ensure_packed(e);
    if (stem) debug_stem_col(e, c, reinterpret_cast<const float*>(x_dev), imgs, groups);
    const Prologue pro{psc_dev, psh_dev, gate_dev};
    if (op == 0) {
        ARGCHK(x_dev, "x");
        conv_fwd(e, e->main, conv, e->student, {reinterpret_cast<const float*>(x_dev)}, {reinterpret_cast<float*>(out_dev)}, imgs, groups,
                 {.stats = stats_dev ? e->ws_stats : nullptr, .pro = pro});
        if (stats_dev) RCCHK(debug_fold_stats(e, conv, groups, stats_dev));
    } else if (op == 1) {
        ARGCHK(dy_dev, "dy");
        conv_dgrad(e, e->main, conv, {reinterpret_cast<const float*>(dy_dev)}, reinterpret_cast<float*>(out_dev), imgs,
                   {.res = reinterpret_cast<const float*>(x_dev)});      // x_dev = optional residual [npix][cin_p] bf16
    } else if (op == 2) {
        ARGCHK(x_dev && dy_dev, "x/dy");
        conv_wgrad(e, e->main, conv, {reinterpret_cast<const float*>(x_dev)}, {reinterpret_cast<const float*>(dy_dev)}, imgs, pro,
                   (imgs / groups) * c.hout * c.wout);
        HIPCHK(hipMemcpyAsync(out_dev, e->grad + c.w_off, c.w_numel * 4, hipMemcpyDeviceToDevice, e->main.st));
    } else {
        ARGCHK(false, "op");
    }
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_debug_pw_fwd(fm_engine* e, int32_t conv, const void* x_dev, void* out_dev, int32_t imgs, int32_t groups,
                    const float* scale_dev, const float* shift_dev, const void* res_dev, int32_t act, const float* psc_dev,
                    const float* psh_dev, const float* gate_dev, float* stats_dev)
{
    ARGCHK(e && x_dev && out_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(e->precision == 1 && e->model == 1, "fm_debug_pw_fwd works on bf16 tensors: an EfficientNet-B0 engine with precision 1");
    Conv& c = e->convs[conv];
    const bool stem = c.cin == 3;
    ARGCHK(c.k == 1 || stem, "a 1x1 convolution or the stem");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs/groups");
    ARGCHK(act == 0 || act == 2, "act: 0 none / 2 swish");
    // the forms the engine's graphs use (fm_debug_conv_fwd's rules on the bf16 kernels); nothing else has a caller
    ARGCHK(!scale_dev == !shift_dev, "scale and shift come together");
    ARGCHK(!psc_dev == !psh_dev, "psc and psh come together");
    const bool epi = scale_dev != nullptr, pro = gate_dev != nullptr;
    ARGCHK(epi || (!res_dev && act == 0), "res / act belong to the eval epilogue: give scale and shift");
    ARGCHK(!epi || (!stats_dev && groups == 1), "the eval epilogue runs without statistics on one group");
    ARGCHK(pro || !psc_dev, "psc / psh without a gate");
    ARGCHK(!stem || (!res_dev && !pro), "no graph hands the stem a residual or an operand prologue");
    ARGCHK(!(epi && psc_dev), "the eval forward carries the gate-only prologue");
    ensure_packed(e);
    if (stem) debug_stem_col(e, c, reinterpret_cast<const float*>(x_dev), imgs, groups);
    const Prologue pr{psc_dev, psh_dev, gate_dev};
    conv_fwd(e, e->main, conv, e->student, {reinterpret_cast<const float*>(x_dev)}, {reinterpret_cast<float*>(out_dev)}, imgs, groups,
             {stats_dev ? e->ws_stats : nullptr, pr, {scale_dev, shift_dev, {reinterpret_cast<const float*>(res_dev)}, act}});
    if (stats_dev) RCCHK(debug_fold_stats(e, conv, groups, stats_dev));
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_debug_proj_bwd(fm_engine* e, int32_t conv, int32_t phase, const void* dyp_dev, const void* yd_dev, const float* bn_dev,
                      const float* gate_dev, const float* ds_dev, int32_t imgs, int32_t groups, void* out_dev, float* pool5_dev)
{
    ARGCHK(e && out_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(e->model == 1 && e->convs[conv].k == 1, "an EfficientNet engine and a 1x1 convolution");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs/groups");
    ARGCHK(dyp_dev && yd_dev && bn_dev && gate_dev && (phase == 0 ? pool5_dev != nullptr : ds_dev != nullptr), "operands");
    Conv& c = e->convs[conv];
    ensure_packed(e);
    const int L = c.cin_p;
    const int nch = proj_bwd_nch(e, c, imgs);
    ARGCHK(nch > 0, "shape not handled by the fused project backward");
    const float* bn = bn_dev;
    const size_t gl = (size_t)groups * L;
    const BnCoef coef{bn, bn + gl, bn + 2 * gl, bn + 3 * gl, bn + 4 * gl, bn + 5 * gl, bn + 6 * gl};
    const int sk = launch_proj_bwd(e, e->main, c, phase, dyp_dev, yd_dev, out_dev, coef, gate_dev, ds_dev, imgs, imgs / groups, nch);
    ARGCHK(sk > 0, "launch refused");
    if (phase == 0) {
        k_reduce_slabs(e->main.ws_slab, reinterpret_cast<float*>(out_dev), sk, (int64_t)c.w_numel, e->main.st);
        std::vector<float> h((size_t)imgs * nch * 5 * L), o((size_t)imgs * 5 * L);
        HIPCHK(hipMemcpyAsync(h.data(), e->acts.se_pool, h.size() * 4, hipMemcpyDeviceToHost, e->main.st));
        HIPCHK(hipStreamSynchronize(e->main.st));
        for (int i = 0; i < imgs; ++i)
            for (int k = 0; k < 5 * L; ++k) {
                double sum = 0;
                for (int t = 0; t < nch; ++t) sum += h[((size_t)i * nch + t) * 5 * L + k];
                o[(size_t)i * 5 * L + k] = (float)sum;
            }
        HIPCHK(hipMemcpy(pool5_dev, o.data(), o.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_debug_exp_bwd(fm_engine* e, int32_t conv, const void* da_dev, const void* ye_dev, const void* x_dev, const void* res_dev,
                     const float* bn_dev, int32_t imgs, int32_t groups, void* dx_dev, float* dw_dev)
{
    ARGCHK(e && da_dev && ye_dev && x_dev && bn_dev && dx_dev && dw_dev && conv >= 0 && conv < (int)e->convs.size(), "operands");
    ARGCHK(e->model == 1 && e->convs[conv].k == 1, "an EfficientNet engine and a 1x1 convolution");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && groups <= 2 && imgs % groups == 0, "imgs/groups");
    Conv& c = e->convs[conv];
    ensure_packed(e);
    const float* bn = bn_dev;
    const size_t gl = (size_t)groups * c.cout_p;
    const BnCoef coef{bn + 3 * gl, bn + 4 * gl, nullptr, nullptr, bn, bn + gl, bn + 2 * gl};
    const int sk = launch_exp_bwd(e, e->main, c, da_dev, ye_dev, x_dev, res_dev, dx_dev, coef, imgs, groups);
    ARGCHK(sk > 0, "shape not handled by the fused expand backward");
    k_reduce_slabs(e->main.ws_slab, dw_dev, sk, (int64_t)c.w_numel, e->main.st);
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_debug_optim_arena(fm_engine* e, int32_t which, float** dev_ptr, int64_t* numel)
{
    ARGCHK(e && dev_ptr && numel && which >= 0 && which <= 3, "null / which");
    if (which == 2 && !e->gacc) {
        DALLOC(e->gacc, e->NP);
        HIPCHK(hipMemsetAsync(e->gacc, 0, e->NP * 4, e->main.st));
    }
    *dev_ptr = which == 0 ? e->adam_m : (which == 1 ? e->adam_v : (which == 2 ? e->gacc : e->grad));
    *numel = (int64_t)e->NP;
    return FM_OK;
}

int fm_debug_entry_spans(fm_engine* e, int64_t* off_len, int32_t n_entries)
{
    ARGCHK(e && off_len && n_entries == (int32_t)e->entries.size(), "null / entry count");
    // a parameter's span as the table's chunks give it: the first one's begin, the sum of their lengths
    for (int32_t i = 0; i < n_entries; ++i) {
        off_len[2 * i] = -1; off_len[2 * i + 1] = 0;
        if (!is_param(e, e->entries[i])) continue;
        const ArenaEntry& a = e->tab.ent[e->tab.ent_of[i]];
        off_len[2 * i] = e->tab.chunks[a.chunk0].begin;
        for (int j = 0; j < a.nchunks; ++j) off_len[2 * i + 1] += e->tab.chunks[a.chunk0 + j].len;
    }
    return FM_OK;
}

int fm_debug_get_grads(fm_engine* e, float* host_f32)
{
    ARGCHK(e && host_f32, "null");
    RCCHK(arena_to_state_dict(e, e->grad, e->stage_sd, true));
    HIPCHK(hipMemcpyAsync(host_f32, e->stage_sd, (size_t)e->nf_sd * 4, hipMemcpyDeviceToHost, e->main.st));
    HIPCHK(hipStreamSynchronize(e->main.st));
    return FM_OK;
}

int fm_profile_ops(fm_engine* e, int32_t enable, char* buf, int32_t cap)
{
    ARGCHK(e, "null engine");
    HIPCHK(hipStreamSynchronize(e->main.st));
    for (auto& p : e->opevs) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) { e->op_ms[p.id] += t; e->op_n[p.id] += 1; }
        e->ev_free.push_back(p.a); e->ev_free.push_back(p.b);
    }
    e->opevs.clear();
    if (buf && cap > 0) {
        std::string out;
        char line[160];
        for (size_t i = 0; i < e->op_names.size(); ++i) {
            snprintf(line, sizeof line, "%s\t%lld\t%.6f\n", e->op_names[i].c_str(), (long long)e->op_n[i], e->op_ms[i]);
            out += line;
        }
        snprintf(buf, (size_t)cap, "%s", out.c_str());
        e->op_names.clear(); e->op_ms.clear(); e->op_n.clear();
    }
    e->oprof = enable != 0;
    return FM_OK;
}

int fm_debug_num_convs(fm_engine* e) { return e ? (int)e->convs.size() : 0; }

int fm_debug_activation(fm_engine* e, int32_t kind, int32_t block, int32_t imgs, float* host_nhwc, int32_t* dims4)
{
    ARGCHK(e && dims4 && e->model == 0, "ResNet-18 engine only");
    ARGCHK(block >= 0 && block < (int)e->blocks.size() && (kind == 0 || kind == 1), "kind/block");
    ARGCHK(imgs >= 1 && imgs <= e->maxB, "imgs");
    const Out t = kind == 0 ? e->acts.blk[block].z1 : e->acts.blk[block].out;
    const Conv& c = e->convs[e->blocks[block].c1];
    dims4[0] = imgs; dims4[1] = c.hout; dims4[2] = c.wout; dims4[3] = c.cout;
    if (host_nhwc) {
        // planes mode: z1 / out (all blocks but the last) live only as planes: re-form the fp32 values in the idle fp32 buffer
        if (e->planes && (kind == 0 || block + 1 < (int)e->blocks.size()))
            k_planes_to_f32(t.p, t.f, (long long)imgs * c.hout * c.wout, c.cout, e->main.st);
        HIPCHK(hipMemcpyAsync(host_nhwc, t.f, (size_t)imgs * c.hout * c.wout * c.cout * 4,
                              hipMemcpyDeviceToHost, e->main.st));
        HIPCHK(hipStreamSynchronize(e->main.st));
    }
    return FM_OK;
}

int fm_debug_lose_part(int32_t on)
{
    pconv_debug_lose_part(on);
    return FM_OK;
}

// ---- lane-order test hooks ----
static void lane_point_armed(fm_engine* e, int lane)
{
    fm_engine::LaneDbg& d = e->ldbg;
    const int64_t pos = d.points[lane]++;
    if (d.fired || lane != d.lane || pos != d.at || d.micros <= 0) return;
    d.fired = true;
    // >= 0.8 us per sleep iteration: three per microsecond cover the time asked for, and end the kernel within a few times it
    k_lane_delay(d.ticks, 3 * d.micros, lane ? e->side.st : e->main.st);
}

int fm_debug_lane_delay(fm_engine* e, int32_t lane, int64_t at, int32_t micros)
{
    ARGCHK(e, "null engine");
    ARGCHK(lane == 0 || lane == 1, "fm_debug_lane_delay: lane is 0 (main) or 1 (side)");
    ARGCHK(lane == 0 || e->side_ok, "fm_debug_lane_delay: lane 1 on a handle without a side stream");
    ARGCHK(at >= 0, "fm_debug_lane_delay: at >= 0");
    ARGCHK(micros >= 0 && micros <= FM_LANE_DELAY_MAX_US, "fm_debug_lane_delay: 0 <= micros <= FM_LANE_DELAY_MAX_US");
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        khz = 100000;                  // wall_clock64() counts at 100 MHz on CDNA
    fm_engine::LaneDbg& d = e->ldbg;
    const uint32_t drop = d.drop;      // the dropped waits are a switch of their own
    d = fm_engine::LaneDbg{};
    d.drop = drop;
    d.armed = true;
    d.lane = lane; d.at = at; d.micros = micros;
    d.ticks = (int64_t)micros * khz / 1000;
    return FM_OK;
}

int fm_debug_lane_points(fm_engine* e, int64_t* out16, int32_t disarm)
{
    ARGCHK(e && out16, "null");
    fm_engine::LaneDbg& d = e->ldbg;
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    out16[0] = d.points[0]; out16[1] = d.points[1]; out16[2] = d.fired;
    for (int k = 0; k < FM_WAIT_KINDS; ++k) { out16[3 + k] = d.waits[k]; out16[3 + FM_WAIT_KINDS + k] = d.skipped[k]; }
    if (disarm) d.armed = false;
    return FM_OK;
}

int fm_debug_drop_wait(fm_engine* e, int32_t which, int32_t on)
{
    ARGCHK(e, "null engine");
    ARGCHK(which >= 0 && which < FM_WAIT_KINDS, "fm_debug_drop_wait: unknown wait kind");
    if (on) e->ldbg.drop |= 1u << which;
    else e->ldbg.drop &= ~(1u << which);
    return FM_OK;
}

int fm_debug_stem_masks(fm_engine* e, int32_t imgs, int32_t groups, uint8_t* relu_bits_host, uint8_t* argmax_host)
{
    ARGCHK(e && e->model == 0 && !e->precision, "ResNet-18 engine only");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs / groups");
    const Conv& c0 = e->convs[0];
    const int64_t pix = (int64_t)imgs * c0.hout * c0.wout;
    if (relu_bits_host) {
        uint8_t* bits = nullptr;
        HIPCHK(hipMalloc(&bits, (size_t)pix * 8));
        k_stem_relu_bits(e->acts.stem_y, e->bns[0].scale, e->bns[0].shift, bits, groups, pix / groups, 64, e->main.st);
        hipError_t rc = hipMemcpyAsync(relu_bits_host, bits, (size_t)pix * 8, hipMemcpyDeviceToHost, e->main.st);
        if (rc == hipSuccess) rc = hipStreamSynchronize(e->main.st);
        (void)hipFree(bits);
        HIPCHK(rc);
    }
    if (argmax_host) {
        HIPCHK(hipMemcpyAsync(argmax_host, e->idx0, (size_t)imgs * (c0.hout / 2) * (c0.wout / 2) * 64, hipMemcpyDeviceToHost, e->main.st));
        HIPCHK(hipStreamSynchronize(e->main.st));
    }
    return FM_OK;
}

int fm_debug_block_dgrad(fm_engine* e, int32_t block, const float* dy1_dev, const float* dyd_dev, float* dx_dev, int32_t imgs)
{
    ARGCHK(e && dy1_dev && dyd_dev && dx_dev, "null tensor");
    ARGCHK(e->model == 0 && !e->precision, "fm_debug_block_dgrad: a precision-0 ResNet-18 engine");
    ARGCHK(block >= 0 && block < (int)e->blocks.size() && e->blocks[block].ds >= 0, "block has no downsample");
    ARGCHK(imgs >= 1 && imgs <= e->maxB, "imgs");
    ensure_packed(e);
    const Block& blk = e->blocks[block];
    if (!block_dgrad(e, e->main, blk.c1, blk.ds, {dy1_dev}, {dyd_dev}, dx_dev, imgs)) {     // (the fp32-operand engine: its two calls)
        conv_dgrad(e, e->main, blk.ds, {dyd_dev}, dx_dev, imgs);
        conv_dgrad(e, e->main, blk.c1, {dy1_dev}, dx_dev, imgs, {.acc_cls0 = true});
    }
    return FM_OK;
}

int fm_debug_conv_info(fm_engine* e, int32_t conv, int32_t* info16)
{
    ARGCHK(e && info16 && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    const Conv& c = e->convs[conv];
    const int v[16] = {c.cin, c.cout, c.k, c.stride, c.pad, c.hin, c.win, c.hout, c.wout, c.cin_p, c.Kw, c.kw_p,
                       c.cout_p, 0, 0, 0};
    memcpy(info16, v, sizeof v);
    return FM_OK;
}

int fm_debug_conv(fm_engine* e, int32_t op, int32_t conv, const float* x_dev, const float* dy_dev, float* out_dev,
                  int32_t imgs, int32_t groups, float* stats_dev)
{
    ARGCHK(e && out_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(!e->precision, "fm_debug_conv works on fp32 tensors: create the engine with precision 0");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs/groups");
    Conv& c = e->convs[conv];
    if (c.stem3 && x_dev)       // the packed stem reads the framed copy of its [imgs][H][W][3] input
        k_frame_nhwc3(x_dev, e->x3, imgs, c.hin, c.win, c.Hp, c.Wp, 3, 3, 1, e->main.st, e->stem_rows ? e->x3p : nullptr, e->x3p_plane_elems);
    ensure_packed(e);           // the forward reads the weight planes, the data gradient the transposed packs
    if (op == 0) {
        ARGCHK(x_dev, "x");
        conv_fwd(e, e->main, conv, e->student, {x_dev}, {out_dev}, imgs, groups, {.stats = stats_dev ? e->ws_stats : nullptr});
        if (stats_dev) RCCHK(debug_fold_stats(e, conv, groups, stats_dev));
    } else if (op == 1) {
        ARGCHK(dy_dev && (c.ncls > 0 || c.cin == 3), "dgrad unavailable for this conv");
        ensure_packed(e);
        if (c.cin == 3) {           // the stem: stem_dgrad.hip with its NHWC store, dx [imgs][hin][win][3]
            RCCHK(ensure_stem_dpack(e));
            stem_dgrad(e, e->main, dy_dev, out_dev, imgs, true);
        } else conv_dgrad(e, e->main, conv, {dy_dev}, out_dev, imgs);
    } else if (op == 2) {
        ARGCHK(x_dev && dy_dev, "x/dy");
        conv_wgrad(e, e->main, conv, {x_dev}, {dy_dev}, imgs);
        HIPCHK(hipMemcpyAsync(out_dev, e->grad + c.w_off, c.w_numel * 4, hipMemcpyDeviceToDevice, e->main.st));
    } else {
        ARGCHK(false, "op");
    }
    return FM_OK;
}

int fm_debug_conv_fwd(fm_engine* e, int32_t conv, const float* x_dev, float* out_dev, int32_t imgs, int32_t groups,
                      const float* scale_dev, const float* shift_dev, const float* res_dev, int32_t act, const float* psc_dev,
                      const float* psh_dev, const float* gate_dev, float* stats_dev)
{
    ARGCHK(e && x_dev && out_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(!e->precision, "fm_debug_conv_fwd works on fp32 tensors: create the engine with precision 0");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && groups >= 1 && imgs % groups == 0, "imgs/groups");
    ARGCHK(act >= 0 && act <= 2, "act");
    Conv& c = e->convs[conv];
    // the three forms the engine's graphs use; everything else would end in conv_fwd's deferred-error branches or in a kernel
    // instantiation that does not exist
    ARGCHK(!scale_dev == !shift_dev, "scale and shift come together");
    ARGCHK(!psc_dev == !psh_dev, "psc and psh come together");
    const bool epi = scale_dev != nullptr, pro = gate_dev != nullptr;
    ARGCHK(epi || (!res_dev && act == 0), "res / act belong to the eval epilogue: give scale and shift");
    ARGCHK(!epi || (!stats_dev && groups == 1), "the eval epilogue runs without statistics on one group");
    ARGCHK(!(c.cin == 3 && res_dev), "no graph hands a stem a residual (the stem_rows kernel has no such operand)");
    ARGCHK(pro || !psc_dev, "psc / psh without a gate");
    if (pro) {
        ARGCHK(e->model == 1 && c.k == 1 && c.stride == 1 && conv1x1_stream_takes(c.cin_p, c.cout_p, c.cout_p),
               "an operand prologue needs a 1x1 convolution of an EfficientNet handle that streams through conv1x1.hip");
        ARGCHK(psc_dev ? (stats_dev && !epi) : !stats_dev,
               "prologue forms: gate alone without statistics, or psc + psh + gate with statistics and no epilogue");
    }
    if (e->planes && c.cin != 3)        // planes mode: the per-tap planes kernel with the operand's planes in the scratch buffer
        ARGCHK(conv_uses_pconv(e, c, imgs) && (size_t)imgs * c.hin * c.win * c.cin_p * 3 <= e->xp_scratch_elems,
               "shape outside the planes kernel");
    if (c.stem3)                // the packed stem reads the framed copy of its [imgs][H][W][3] input
        k_frame_nhwc3(x_dev, e->x3, imgs, c.hin, c.win, c.Hp, c.Wp, 3, 3, 1, e->main.st, e->stem_rows ? e->x3p : nullptr, e->x3p_plane_elems);
    ensure_packed(e);
    const Prologue pr{psc_dev, psh_dev, gate_dev};
    conv_fwd(e, e->main, conv, e->student, {x_dev}, {out_dev}, imgs, groups,
             {stats_dev ? e->ws_stats : nullptr, pr, {scale_dev, shift_dev, {res_dev}, act}});
    if (stats_dev) RCCHK(debug_fold_stats(e, conv, groups, stats_dev));
    HIPCHK(hipGetLastError());
    return FM_OK;
}

int fm_debug_conv_planes(fm_engine* e, int32_t conv, const uint16_t* xp_dev, int32_t imgs, const float* scale_dev,
                         const float* shift_dev, const float* res_dev, const uint16_t* resp_dev, int32_t relu, float* out_dev,
                         uint16_t* outp_dev)
{
    ARGCHK(e && xp_dev && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(e->model == 0 && !e->precision && e->planes, "fm_debug_conv_planes: a planes-mode precision-0 ResNet-18 engine");
    ARGCHK(scale_dev && shift_dev, "the eval epilogue needs scale and shift");
    ARGCHK(imgs >= 1 && imgs <= e->maxB, "imgs");
    ARGCHK(relu == 0 || relu == 1, "relu");
    ARGCHK(!(res_dev && resp_dev), "one residual form: fp32 or planes");
    ARGCHK(out_dev || outp_dev, "an output: fp32, planes or both");
    Conv& c = e->convs[conv];
    ARGCHK(c.cin != 3 && conv_uses_pconv(e, c, imgs), "a convolution the planes kernel runs (not the stem)");
    ensure_packed(e);
    // as forward_eval: the operand's planes, one group, no statistics, the output and the residual in either form
    conv_fwd(e, e->main, conv, e->student, {.p = xp_dev}, {out_dev, outp_dev}, imgs, 1, {.epi = {scale_dev, shift_dev, {res_dev, resp_dev}, relu}});
    HIPCHK(hipStreamSynchronize(e->main.st));
    STEP_DONE(e);
    return FM_OK;
}

int fm_debug_conv_arm(fm_engine* e, int32_t op, int32_t conv, int32_t imgs)
{
    ARGCHK(e && conv >= 0 && conv < (int)e->convs.size(), "conv index");
    ARGCHK(!e->precision, "fm_debug_conv_arm: a precision-0 engine");
    ARGCHK(imgs >= 1 && imgs <= e->maxB && op >= 0 && op <= 2, "imgs / op");
    const Conv& c = e->convs[conv];
    if (op == 1 && c.cin == 3) return FM_ARM_STEM_DGRAD;        // fm_debug_conv's data gradient of the stem: its own kernel
    ARGCHK(op != 1 || c.ncls > 0, "dgrad unavailable for this conv");
    switch (op == 0 ? fwd_arm(e, c, imgs) : (op == 1 ? dgrad_arm(e, c, imgs) : wgrad_arm(e, c, imgs))) {
    case Arm::StemRows: return FM_ARM_STEM_ROWS;
    case Arm::PconvTs: return FM_ARM_PCONV_TS;
    case Arm::PconvTap: return FM_ARM_PCONV_TAP;
    case Arm::Igemm: return FM_ARM_IGEMM;
    case Arm::IgemmStem: return FM_ARM_IGEMM_STEM;
    case Arm::Pwgrad: return FM_ARM_PWGRAD;
    case Arm::PwgradRing: return FM_ARM_PWGRAD_RING;
    case Arm::WgradSkinny: return FM_ARM_WGRAD_SKINNY;
    case Arm::WgradGeneric:
    case Arm::WgradGenericStem: return FM_ARM_WGRAD_GENERIC;
    default: break;                     // None (the bf16 pointwise arms need precision 1)
    }
    g_err = "bad argument: no kernel for this shape in planes mode";
    return FM_ERR_ARG;
}

int fm_debug_ew(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc)
{
    ARGCHK(e && p && d && sc, "null argument");
    ARGCHK(e->model == 0 && !e->precision, "fm_debug_ew: a precision-0 ResNet-18 engine");
    hipStream_t s = e->main.st;
    auto F = [&](int i) { return static_cast<float*>(p[i]); };
    auto U = [&](int i) { return static_cast<unsigned short*>(p[i]); };
    auto B = [&](int i) { return static_cast<uint8_t*>(p[i]); };
    auto need = [&](std::initializer_list<int> idx) { for (int i : idx) if (!p[i]) return false; return true; };
    auto pos = [&](int n) { for (int i = 0; i < n; ++i) if (d[i] < 1) return false; return true; };
    switch (op) {
    case FM_EW_SPLIT_PLANES:
    case FM_EW_PLANES_TO_F32:
        ARGCHK(need({0, 1}) && pos(2) && d[1] % 32 == 0, "planes: C % 32");
        if (op == FM_EW_SPLIT_PLANES) k_split_planes(F(0), U(1), d[0], d[1], s);
        else k_planes_to_f32(U(0), F(1), d[0], d[1], s);
        break;
    case FM_EW_BN_FINALIZE:
        ARGCHK(need({0, 1, 2, 5, 6, 7, 8}) && pos(4) && (!p[3] == !p[4]), "bn_finalize operands");
        k_bn_finalize(F(0), d[0], d[1], d[2], d[3], F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), sc[0], sc[1], s,
                      static_cast<const int*>(p[9]));
        break;
    case FM_EW_BN_FINALIZE_FROZEN:
        ARGCHK(need({0, 1, 2, 3, 4, 5, 6, 7}) && pos(2), "bn_finalize_frozen operands");
        k_bn_finalize_frozen(d[0], d[1], F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), sc[0], s, static_cast<const int*>(p[8]));
        break;
    case FM_EW_BN_EVAL_AFFINE:
        ARGCHK(need({0, 1, 2, 3, 4, 5}) && pos(1), "bn_eval_affine operands");
        k_bn_eval_affine(F(0), F(1), F(2), F(3), F(4), F(5), d[0], sc[0], s);
        break;
    case FM_EW_BN_APPLY:
    case FM_EW_BN_APPLY_PLANES: {
        const bool pl = op == FM_EW_BN_APPLY_PLANES;
        ARGCHK(need({0, 1, 2}) && pos(3) && d[2] % 4 == 0, "bn_apply: C % 4");
        ARGCHK(!p[4] || (p[5] && p[6]), "bn_apply: y2 needs scale2 / shift2");
        if (pl) {
            ARGCHK(d[2] % 32 == 0 && p[8] && !(p[3] && p[9]), "bn_apply_planes: C % 32, outp, one residual form");
            k_bn_apply_planes(F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), U(8), d[0], d[1], d[2], d[3], s, U(9));
        } else {
            ARGCHK(p[7], "bn_apply: out");
            k_bn_apply(F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), d[0], d[1], d[2], d[3], s);
        }
        break;
    }
    case FM_EW_STEM_POOL:
    case FM_EW_STEM_POOL_PLANES: {
        const bool pl = op == FM_EW_STEM_POOL_PLANES;
        ARGCHK(p[0] && (!p[1] == !p[2]) && pos(5) && d[4] % 4 == 0 && d[2] % 2 == 0 && d[3] % 2 == 0, "stem_pool: C % 4, even H, W");
        if (pl) {
            ARGCHK(d[4] % 32 == 0 && p[5], "stem_pool_planes: C % 32, pooledp");
            k_stem_pool_planes(F(0), F(1), F(2), F(3), B(4), U(5), d[0], d[1], d[2], d[3], d[4], s);
        } else {
            ARGCHK(p[3], "stem_pool: pooled");
            k_stem_pool(F(0), F(1), F(2), F(3), B(4), d[0], d[1], d[2], d[3], d[4], s);
        }
        break;
    }
    case FM_EW_STEM_POOL_BWD:
        ARGCHK(need({0, 1, 2, 3}) && pos(4) && d[3] % 4 == 0 && d[1] % 2 == 0 && d[2] % 2 == 0, "stem_pool_bwd: C % 4, even H, W");
        k_stem_pool_bwd(F(0), F(1), B(2), F(3), d[0], d[1], d[2], d[3], s);
        break;
    case FM_EW_STEM_POOL_BN_REDUCE:
        ARGCHK(need({0, 1, 2, 3, 4, 5, 6, 7, 8}) && pos(5) && d[4] % 4 == 0 && d[4] <= 1024 && 1024 % d[4] == 0 && d[2] % 2 == 0 &&
                   d[3] % 2 == 0, "stem_pool_bn_reduce: C a power of two in 4 .. 1024, even H, W");
        k_stem_pool_bn_reduce(F(0), F(1), B(2), F(3), F(4), F(5), F(6), d[0], d[1], d[2], d[3], d[4], s, F(7), F(8));
        break;
    case FM_EW_STEM_POOL_BN_APPLY:
        ARGCHK(need({0, 1, 2, 3, 4, 5, 6, 7}) && pos(5) && d[4] % 4 == 0 && d[2] % 2 == 0 && d[3] % 2 == 0,
               "stem_pool_bn_apply: C % 4, even H, W");
        k_stem_pool_bn_apply(F(0), F(1), B(2), F(3), F(4), F(5), F(6), F(7), d[0], d[1], d[2], d[3], d[4], s);
        break;
    case FM_EW_BN_BWD_REDUCE:
        ARGCHK(need({0, 2, 3, 4, 5}) && pos(3) && d[2] % 4 == 0 && d[2] <= 1024 && 1024 % d[2] == 0,
               "bn_bwd_reduce: C a power of two in 4 .. 1024");
        ARGCHK((!p[6] == !p[7]) && (!p[8] || d[2] % 32 == 0), "bn_bwd_reduce: mask_scale with mask_shift, zh needs C % 32");
        k_bn_bwd_reduce(F(0), F(1), F(2), F(3), F(4), F(5), d[0], d[1], d[2], s, F(6), F(7), U(8));
        break;
    case FM_EW_BN_BWD_FINALIZE:
        ARGCHK(need({0, 1, 2, 3, 4, 5, 6, 7, 8}) && pos(4), "bn_bwd_finalize operands");
        k_bn_bwd_finalize(F(0), d[0], d[1], d[2], d[3], F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), s, d[4] != 0);
        break;
    case FM_EW_BN_BWD_APPLY:
    case FM_EW_BN_BWD_APPLY_PLANES: {
        const bool pl = op == FM_EW_BN_BWD_APPLY_PLANES;
        ARGCHK(need({0, 2, 3, 4, 5}) && pos(3) && d[2] % 4 == 0 && (!p[8] == !p[9]), "bn_bwd_apply: C % 4, mask_scale with mask_shift");
        if (pl) {
            ARGCHK(d[2] % 32 == 0 && p[10], "bn_bwd_apply_planes: C % 32, dyp");
            k_bn_bwd_apply_planes(F(0), F(1), F(2), F(3), F(4), F(5), F(6), U(10), F(7), d[0], d[1], d[2], s, F(8), F(9), U(11));
        } else {
            ARGCHK(p[6], "bn_bwd_apply: dy");
            k_bn_bwd_apply(F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), d[0], d[1], d[2], s, F(8), F(9));
        }
        break;
    }
    default:
        ARGCHK(false, "op");
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return FM_OK;
}

// ---- fm_debug_eff: the depthwise / squeeze-excite launchers of effnet.hip on caller tensors ---------------------------------------
// shared argument contract of fm_debug_eff and fm_debug_eff_ws (nullptr = fine, else the complaint)
static const char* eff_dims_bad(int32_t op, const int32_t* d)
{
    auto pos = [&](int a, int b) { for (int i = a; i < b; ++i) if (d[i] < 1) return false; return true; };
    if (op == FM_EFF_DW_FWD || op == FM_EFF_DW_DGRAD || op == FM_EFF_DW_WGRAD) {
        if (d[0] != DT_F32 && d[0] != DT_BF16) return "dt";
        if (!pos(1, 7) || d[12] < 1) return "a dimension < 1";
        if (d[6] % 4) return "C % 4";
        if (d[7] != 3 && d[7] != 5) return "K is 3 or 5";
        if (d[8] != 1 && d[8] != 2) return "stride is 1 or 2";
        if (d[4] != (d[2] + d[8] - 1) / d[8] || d[5] != (d[3] + d[8] - 1) / d[8]) return "Ho, Wo = ceil(Hi, Wi / stride)";
        if (d[9] < 0 || d[9] >= d[7] || d[10] < 0 || d[10] >= d[7]) return "pad_t, pad_l in 0 .. K-1";
        if (d[11] < 0 || d[11] > 2) return "act";
        if ((int64_t)d[1] * d[2] * d[3] * d[6] >= ((int64_t)1 << 30)) return "tensor too large";
        return nullptr;
    }
    if (op == FM_EFF_SE_WGRAD) {
        if (!pos(0, 3)) return "a dimension < 1";
        if (d[1] % 4) return "C % 4";
        if (d[2] > se_wgrad_max_cs()) return "Cs beyond the weight-gradient kernel's accumulators";
        return nullptr;
    }
    if (op == FM_EFF_SE_FWD || op == FM_EFF_SE_SCALE || op == FM_EFF_SE_BWD_BN1) {
        if (d[0] != DT_F32 && d[0] != DT_BF16) return "dt";
        if (!pos(1, 6) || d[6] < 0) return "a dimension < 1";
        if (d[3] % (d[0] == DT_BF16 ? 8 : 4)) return "C % 4 (C % 8 in bf16 storage)";
        if (d[1] % d[5]) return "imgs % ipg";
        if (d[3] + d[4] > 12288) return "C + Cs beyond the block's LDS";
        if ((int64_t)d[1] * d[2] * d[3] >= ((int64_t)1 << 30)) return "tensor too large";
        return nullptr;
    }
    if (op == FM_EFF_BNACT_APPLY || op == FM_EFF_CHAN_REDUCE || op == FM_EFF_BNACT_BWD_APPLY) {
        // d = {ty, ta, groups, pix_per_group, HW, C, mode, act}
        if ((d[0] != DT_F32 && d[0] != DT_BF16) || (d[1] != DT_F32 && d[1] != DT_BF16)) return "ty / ta";
        if (d[0] == DT_BF16 && d[1] == DT_F32) return "(ty, ta) is (f32, f32), (f32, bf16) or (bf16, bf16)";
        if (!pos(2, 6)) return "a dimension < 1";
        if (d[5] % ((d[0] == DT_BF16 && d[1] == DT_BF16) ? 8 : 4)) return "C % 4 (C % 8 when both types are bf16)";
        if (d[3] % d[4]) return "pix_per_group % HW";
        if (op == FM_EFF_CHAN_REDUCE ? (d[6] != 0 && d[6] != 1) : d[6] != 0) return "mode";
        if (op == FM_EFF_BNACT_APPLY ? (d[7] < 0 || d[7] > 2) : (d[7] != 0 && d[7] != 2)) return "act";
        if ((int64_t)d[2] * d[3] * d[5] >= ((int64_t)1 << 30)) return "tensor too large";
        return nullptr;
    }
    return "op";
}

int fm_debug_eff_ws(int32_t op, const int32_t* d, int64_t* floats)
{
    ARGCHK(d && floats, "null argument");
    BADCHK(eff_dims_bad(op, d));
    for (int i = 0; i < FM_EFF_NWS; ++i) floats[i] = 0;
    switch (op) {
    case FM_EFF_DW_FWD:
    case FM_EFF_DW_DGRAD: {
        const bool dg = op == FM_EFF_DW_DGRAD;
        floats[0] = dw_rec_floats(dg, false, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[12]);
        floats[1] = (int64_t)d[12] * dw_stats_tiles() * 2 * d[6];
        floats[2] = dw_rec_floats(dg, true, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], 1);
        floats[3] = dg ? 0 : (int64_t)d[1] * d[6];
        break;
    }
    case FM_EFF_DW_WGRAD:
        floats[0] = dw_wgrad_part_floats(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]);
        floats[1] = (int64_t)d[7] * d[7] * d[6];
        break;
    case FM_EFF_SE_FWD:
        floats[0] = (int64_t)d[1] * (d[6] ? 1 : chan_pool_chunks(d[2])) * d[3];
        break;
    case FM_EFF_SE_SCALE:
        break;
    case FM_EFF_SE_BWD_BN1:
        floats[0] = (int64_t)d[1] * (d[6] > 0 ? d[6] : se_bwd_bn1_chunks(d[2], d[1])) * 5 * d[3];
        floats[1] = (int64_t)(d[1] / d[5]) * se_bwd_bn1_splits(d[5]) * 2 * d[3];
        floats[2] = se_bwd_bn1_splits(d[5]);
        break;
    case FM_EFF_SE_WGRAD:
        floats[1] = se_wgrad_range_floats(d[1], d[2]);
        floats[0] = floats[1] * se_wgrad_splits();
        break;
    case FM_EFF_CHAN_REDUCE:
        floats[0] = (int64_t)d[2] * bn_bwd_blocks(d[3]) * 2 * d[5];
        break;
    case FM_EFF_BNACT_APPLY:
    case FM_EFF_BNACT_BWD_APPLY:
        break;
    }
    return FM_OK;
}

int fm_debug_eff(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc)
{
    (void)sc;                           // reserved: no launcher of this family takes a scalar
    ARGCHK(e && p && d, "null argument");
    ARGCHK(e->model == 1, "fm_debug_eff: an EfficientNet-B0 engine");
    BADCHK(eff_dims_bad(op, d));
    hipStream_t s = e->main.st;
    auto F = [&](int i) { return static_cast<float*>(p[i]); };
    auto need = [&](std::initializer_list<int> idx) { for (int i : idx) if (!p[i]) return false; return true; };
    int32_t* served = static_cast<int32_t*>(p[FM_EFF_NPTR - 1]);          // HOST slot
    bool flag = false;
    switch (op) {
    case FM_EFF_DW_FWD: {
        ARGCHK(need({0, 1, 2}) && (!p[3] == !p[4]), "dw_fwd: x, w, y; scale with shift");
        ARGCHK(p[3] || !d[11], "dw_fwd: act needs scale / shift");
        ARGCHK(!(p[6] && p[7]) && (!p[5] == !(p[6] || p[7])), "dw_fwd: rec with exactly one of stats_out / pool_out");
        ARGCHK(!p[5] || served, "dw_fwd: a request needs the served slot");
        flag = k_dw_fwd(p[0], F(1), p[2], d[0], F(3), F(4), d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], s, F(5),
                        F(6), d[12], F(7));
        break;
    }
    case FM_EFF_DW_DGRAD: {
        ARGCHK(need({0, 1, 2}), "dw_dgrad: dy, w, dx");
        const bool any = p[3] || p[4] || p[5] || p[6] || p[7] || p[8] || p[9];
        ARGCHK(!any || (need({3, 4, 5, 6, 7, 8, 9}) && served), "dw_dgrad: ye comes with mean, istd, scale, shift, rec, stats_out, served");
        flag = k_dw_dgrad(p[0], F(1), p[2], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], s, p[3], F(4), F(5), F(6),
                          F(7), F(8), F(9), d[12]);
        break;
    }
    case FM_EFF_DW_WGRAD:
        ARGCHK(need({0, 1, 2, 3}), "dw_wgrad: dy, x, part, out");
        k_dw_wgrad(p[0], p[1], d[0], F(2), F(3), d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], s);
        break;
    case FM_EFF_SE_FWD:
        ARGCHK(need({3, 4, 5, 6, 7, 8, 9, 10}) && (!p[1] == !p[2]), "se_fwd: operands; scale with shift");
        ARGCHK(d[6] ? !p[1] : p[0] != nullptr, "se_fwd: a unless pooled; pooled sums are of the activation (no scale / shift)");
        k_se_fwd(p[0], d[0], F(1), F(2), d[5], F(3), F(4), F(5), F(6), F(7), F(8), F(9), F(10), d[1], d[2], d[3], d[4], s, d[6] != 0);
        break;
    case FM_EFF_SE_SCALE:
        ARGCHK(need({0, 3, 4}) && (!p[1] == !p[2]), "se_scale: a, gate, out; scale with shift");
        k_se_scale(p[0], d[0], F(1), F(2), d[5], F(3), p[4], d[1], d[2], d[3], s);
        break;
    case FM_EFF_SE_BWD_BN1:
        ARGCHK(need({1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14}), "se_bwd_bn1 operands");
        ARGCHK(p[0] || d[6] > 0, "se_bwd_bn1: dout may be absent only when pool_ws already holds nch_ready records per image");
        k_se_bwd_bn1(p[0], p[1], d[0], F(2), F(3), F(4), F(5), d[5], F(6), F(7), F(8), F(9), F(10), F(11), F(12), F(13), F(14), d[1],
                     d[2], d[3], d[4], s, d[6]);
        break;
    case FM_EFF_SE_WGRAD:
        ARGCHK(need({0, 1, 2, 3, 4, 5}), "se_wgrad operands");
        k_se_wgrad(F(0), F(1), F(2), F(3), F(4), F(5), d[0], d[1], d[2], s);
        break;
    case FM_EFF_BNACT_APPLY:
        ARGCHK(need({0, 1, 2, 5}), "bnact_apply: y, scale, shift, out");
        k_bnact_apply(p[0], d[0], F(1), F(2), p[3], F(4), p[5], d[1], d[2], d[3], d[4], d[5], d[7], s);
        break;
    case FM_EFF_CHAN_REDUCE:
        ARGCHK(need({1, 7}), "chan_reduce: y, part");
        ARGCHK(d[6] == 0 || need({0, 2, 3}), "chan_reduce mode 1: a, mean, istd");
        ARGCHK(d[7] != 2 || (p[4] && p[5]), "chan_reduce: act 2 needs scale / shift");
        ARGCHK(!p[8] == !p[9], "chan_reduce: gate with dsv");
        k_chan_reduce(p[0], d[1], p[1], d[0], F(2), F(3), F(4), F(5), F(6), F(7), d[2], d[3], d[4], d[5], d[6], d[7], F(8), F(9), s);
        break;
    case FM_EFF_BNACT_BWD_APPLY:
        ARGCHK(need({0, 1, 2, 3, 4, 8}), "bnact_bwd_apply: dz, y, ca, cb, cc, dy");
        ARGCHK(d[7] != 2 || (p[5] && p[6]), "bnact_bwd_apply: act 2 needs scale / shift");
        ARGCHK(!p[9] == !p[10], "bnact_bwd_apply: gate with dsv");
        k_bnact_bwd_apply(p[0], d[1], p[1], d[0], F(2), F(3), F(4), F(5), F(6), F(7), p[8], d[2], d[3], d[4], d[5], d[7], F(9), F(10), s);
        break;
    default:
        ARGCHK(false, "op");
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (served) *served = flag ? 1 : 0;
    return FM_OK;
}

// ---- fm_debug_head: the classifier-head and loss launchers of heads.hip on caller tensors ------------------------------------------
int fm_debug_head(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc)
{
    ARGCHK(e && p && d && sc, "null argument");
    hipStream_t s = e->main.st;
    auto F = [&](int i) { return static_cast<float*>(p[i]); };
    auto need = [&](int n) { for (int i = 0; i < n; ++i) if (!p[i]) return false; return true; };
    auto pos = [&](int a, int b) { for (int i = a; i < b; ++i) if (d[i] < 1) return false; return true; };
    auto small = [&](int64_t n) { return n < ((int64_t)1 << 30); };
    switch (op) {
    case FM_HD_AVGPOOL:
        ARGCHK(d[0] == DT_F32 || d[0] == DT_BF16, "avgpool: dt");
        ARGCHK(need(2) && pos(1, 4) && small((int64_t)d[1] * d[2] * d[3]), "avgpool: x, feat; imgs, HW, C >= 1");
        k_avgpool(p[0], d[0], F(1), d[1], d[2], d[3], s);
        break;
    case FM_HD_FC_FWD:
        ARGCHK(need(4) && pos(0, 3) && d[2] <= FM_MAXC && small((int64_t)d[0] * d[1]), "fc_fwd: feat, W, b, logits; imgs, D >= 1, C in 1 .. 32");
        k_fc_fwd(F(0), F(1), F(2), F(3), d[0], d[1], d[2], s);
        break;
    case FM_HD_FC_BWD:
        ARGCHK(d[0] == DT_F32 || d[0] == DT_BF16, "fc_bwd: dt");
        ARGCHK(need(3) && p[4] && p[5] && p[6], "fc_bwd: dz, feat, W, dW, db, dout");
        ARGCHK(pos(1, 5) && d[3] <= FM_MAXC && small((int64_t)d[1] * d[2] * d[4]), "fc_bwd: imgs, D, HW >= 1, C in 1 .. 32");
        k_fc_bwd(F(0), F(1), F(2), F(3), F(4), F(5), p[6], d[0], d[1], d[2], d[3], d[4], s, F(7));
        break;
    case FM_HD_LOSS_BCE:
        ARGCHK(need(5) && pos(0, 2) && d[1] <= FM_MAXC && small((int64_t)d[0] * d[1]), "loss_bce: z, y, pos_w, dz, loss; B >= 1, C in 1 .. 32");
        k_loss_bce(F(0), F(1), to_cv(F(2), d[1]), d[0], d[1], sc[0], F(3), F(4), s);
        break;
    case FM_HD_LOSS_STAGE1:
        ARGCHK(need(6) && pos(0, 2) && d[1] <= FM_MAXC && small((int64_t)d[0] * d[1]),
               "loss_stage1: z, g, y, active, dz, loss; B >= 1, C in 1 .. 32");
        k_loss_stage1(F(0), F(1), F(2), to_cv(F(3), d[1]), d[0], d[1], sc[0], sc[1], F(4), F(5), s);
        break;
    case FM_HD_LOSS_STAGE2:
        ARGCHK(need(5) && pos(0, 2) && d[1] <= FM_MAXC && small((int64_t)d[0] * d[1]),
               "loss_stage2: z, y, distill, dz, loss; B >= 1, C in 1 .. 32");
        k_loss_stage2(F(0), F(1), F(2), d[0], d[1], F(3), F(4), s);
        break;
    case FM_HD_LOSS_FIXMATCH: {
        ARGCHK(need(7) && pos(0, 2) && d[1] <= FM_MAXC && d[2] >= 0 && small((int64_t)d[0] * d[1]),
               "loss_fixmatch: z, y, pos_w, pos_wu, active, dz, loss; B >= 1, C in 1 .. 32");
        ARGCHK(d[0] <= 2048, "loss_fixmatch: B <= 2048 (the confident-row table)");
        int n_neg = 0;
        for (int c = 0; c < d[1]; ++c) n_neg += F(4)[c] == 0.f;
        ARGCHK(n_neg == 0 || d[2] >= 1, "loss_fixmatch: cls_minus_ann >= 1 when a class is missing (the kernel divides by it)");
        k_loss_fixmatch(F(0), F(1), to_cv(F(2), d[1]), to_cv(F(3), d[1]), to_cv(F(4), d[1]), d[0], d[1], n_neg, sc[0], d[2], F(5),
                        F(6), s);
        break;
    }
    default:
        ARGCHK(false, "op");
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return FM_OK;
}

}  // extern "C"
