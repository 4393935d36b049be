/*
 * fedmlp_hip.h -- C ABI of the MI355X-native FedMLP per-client training engine.
 *
 * The reference (szbonaldo/FedMLP) has no FFI layer: its boundary for this path
 * is the Python call surface build_model() / LocalUpdate / FedAvg* (SURVEY.md
 * 8b).  This library is what a ctypes binding of that surface calls; the
 * reference-side stub is shown in INTEGRATION.md.  Plain pointers and sizes
 * only: no torch types, no C++ types, no exceptions across the boundary.
 *
 * Conventions
 *   - One opaque engine per GPU/process; not thread-safe per handle
 *     (the reference drives the model from a single thread, main.py:135).
 *   - Every function returns 0 on success, a negative code on failure;
 *     fm_last_error() returns a human-readable message for the calling thread.
 *   - "dev" pointers are HIP device pointers owned by the caller (the Python
 *     shim passes torch tensor data_ptr()s); "host" pointers are host memory.
 *   - Images are fp32 NCHW [B,3,H,W] exactly as the reference's DataLoader
 *     yields them (dataset/all_dataset.py:73-83); labels/masks fp32 [B,C].
 *   - All work is enqueued on the stream given at fm_create (0 = the null
 *     stream, which is also torch's default stream); nothing synchronises
 *     except fm_sync, fm_get_state, fm_set_state and the *_host getters.
 *   - The model state crosses the boundary in the reference's state_dict
 *     order (torchvision key order, conv weights OIHW): one flat fp32 buffer
 *     + one int64 buffer of num_batches_tracked counters (fedmlp_amd/spec.py).
 */
#ifndef FEDMLP_HIP_H
#define FEDMLP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_MAX_CLASSES 32

#define FM_OK 0
#define FM_ERR_ARG (-1)     /* bad argument / unsupported configuration */
#define FM_ERR_HIP (-2)     /* a HIP runtime call failed                */
#define FM_ERR_STATE (-3)   /* call sequence error                      */

typedef struct fm_engine fm_engine;

typedef struct fm_config {
    int32_t model;        /* 0 = ResNet-18 (model/all_models.py:53-54, 117-120);
                             1 = EfficientNet-B0 (model/all_models.py:73-75, 121-124) */
    int32_t n_classes;    /* args.n_classes, <= FM_MAX_CLASSES                       */
    int32_t in_h, in_w;   /* input spatial size (224 in the reference, >= 32)        */
    int32_t max_images;   /* max images in ONE forward call (views x batch; eval     */
                          /* passes use 4*batch_size, utils/local_training.py:977)   */
    int32_t reserved[3];  /* reserved[0] = activation precision: 0 fp32 (the reference's arithmetic,
                             utils/local_training.py:14 imports autocast and never uses it);
                             1 bf16 activation storage + bf16 MFMA for the 1x1 convolutions, fp32
                             accumulation / BN statistics / master weights / Adam -- EfficientNet-B0
                             only (BASELINE configs[4]).
                             reserved[1] = stream mode: 0 (default) the frozen teacher's forward and the
                             backward's weight gradients are enqueued on an engine-owned side stream that is
                             forked from and joined to `stream` inside every call (same bits as one stream);
                             1 = everything on `stream` (use for per-kernel profiling); 2 = teacher forward on
                             the side stream only.
                             reserved[2] = product form of the fp32 convolution GEMMs, fixed for the handle's life:
                             0 (default) the library default = every fp32 product as six exact bf16 partial products
                             on the bf16 matrix pipe, fp32 accumulation (csrc/split3.h); 1 = products on the fp32
                             matrix pipe; 2 = all nine partial products; 3 = exactly six (what 0 resolves to in the
                             shipped library, but not overridden by the test-only FM_MFMA_SPLIT).  fm_products() reports it. */
    void*   stream;       /* hipStream_t; NULL = null stream                         */
} fm_config;

/* Adam hyper-parameters of utils/local_training.py:636-637 (torch.optim.Adam,
 * coupled L2 weight decay). */
typedef struct fm_adam {
    float lr, beta1, beta2, eps, weight_decay;
} fm_adam;

/* torch.optim.SGD hyper-parameters (autograd path): all >= 0 except dampening; nesterov != 0 needs momentum > 0 and
 * dampening == 0, like torch. */
typedef struct fm_sgd {
    float lr, momentum, dampening, weight_decay;
    int32_t nesterov;
} fm_sgd;

const char* fm_last_error(void);
const char* fm_version(void);

/* ---- lifetime ---------------------------------------------------------- */
int fm_create(const fm_config* cfg, fm_engine** out);
int fm_destroy(fm_engine* e);
int fm_sync(fm_engine* e);

/* ---- state: net.state_dict() / load_state_dict()  (main.py:196, 222) ----- */
/* Sizes of the state_dict-order buffers (fp32 elements, int64 counters). */
int fm_state_sizes(fm_engine* e, int64_t* n_f32, int64_t* n_i64);
int fm_set_state(fm_engine* e, const float* host_f32, const int64_t* host_i64);
int fm_get_state(fm_engine* e, float* host_f32, int64_t* host_i64);
/* The engine-layout device buffer holding every fp32 state entry (parameters
 * then BN running statistics).  FedAvg (utils/FedAvg.py:7-14) is element-wise,
 * so the RCCL all-reduce of main.py:218's aggregation runs on this buffer in
 * place; *numel is its length.  Valid until fm_destroy. */
int fm_state_device(fm_engine* e, float** dev_ptr, int64_t* numel);
/* num_batches_tracked counters (state_dict order): read (set == 0) or overwrite.
 * They never enter the arithmetic (momentum is fixed at 0.1) but FedAvg
 * averages them like every other entry (utils/FedAvg.py:9-13). */
int fm_counters(fm_engine* e, int64_t* host_i64, int32_t set);
/* state *= w  (the n_i / sum(n) pre-scale before the all-reduce SUM). */
int fm_state_scale(fm_engine* e, float w);
/* FedAvg (utils/FedAvg.py:7-14) of K client states that share ONE GPU (main.py:135-218 trains its clients in turn and
 * aggregates their state_dicts in one process): out[j] = ((s_0[j]*n_0 + s_1[j]*n_1) + ...) / sum(n) in the reference's
 * left-to-right order with its roundings (separate fp32 product and sum, IEEE division), so fp32 entries are bit-identical
 * to utils/FedAvg.py run on CPU tensors (what the KAT pins; on CUDA tensors torch divides by multiplying with the reciprocal,
 * which can differ in the last bit).  states_dev: HOST array of K device pointers to engine-layout states (fm_state_device()'s layout and
 * length, e.g. copies of it taken after each client's round); n_host: the K sample counts (dict_len); K <= 16; out_dev may
 * be fm_state_device()'s buffer itself or any of the inputs.  The num_batches_tracked counters stay with the caller
 * (fm_counters). */
int fm_fedavg_fold(fm_engine* e, const float* const* states_dev, const float* n_host, int32_t K, float* out_dev);
/* ---- RSCFed aggregation (utils/FedAvg.py:16-49) over client states that share ONE GPU ------
 * Fed_w (:16-23): the fold above with the reference's Python-float weights: every weight is rounded to fp32 once and the
 * divisor is (float)(sum of the DOUBLE weights), which can differ in the last bit from the fold's sum of rounded weights when
 * the weights are not integers.  Same kernels, K limit, aliasing rule (out_dev may be an input or the engine's state) and
 * roundings as the fold: bit-identical on fp32 entries to Fed_w on CPU tensors. */
int fm_fed_w(fm_engine* e, const float* const* states_dev, const double* w_host, int32_t K, float* out_dev);
/* The per-entry terms of model_dist (:43-49): norms_dev[k * n_entries + j] = || entry j of states_dev[k] - entry j of ref_dev ||_2
 * for every fp32 state_dict entry j in state_dict order (n_entries of them: 102 for ResNet-18; the int64 counters stay with
 * the caller).  ref_dev NULL: the reference is the states' own unweighted mean Fed_w(states, [1]*K), formed element by element
 * in registers with the fold's roundings and never stored, so each state is read once.  Only state_dict elements count: the
 * padding of the engine layout and the gaps between its matrices may hold anything.  The difference is formed in fp32 as
 * torch does, squares and sums in fp64 in a fixed order (no atomics: two calls give the same bits), so each norm is the
 * correctly rounded norm of the fp32 differences to within one fp32 ulp.  model_dist is the fp32 sum of a row, in order, with
 * the counters' terms at their places.  K <= 16; device norms_dev of K * n_entries floats; enqueued on the engine's stream. */
int fm_state_dist(fm_engine* e, const float* const* states_dev, int32_t K, const float* ref_dev, float* norms_dev,
                  int32_t n_entries);
/* ---- FedAvg across ranks as RCCL calls inside the library (one client per GPU) --------------
 * utils/FedAvg.py:7-14 (FedAvg), :51-70 (FedAvg_tao), :72-93 (FedAvg_proto) walk a Python list of
 * client results in one process.  With one process per GPU the same weighted sums are
 * ncclAllReduce(SUM) calls over xGMI, enqueued on the engine's stream.  RCCL is resolved at run
 * time (dlopen); the communicator is the library's own, so a C caller needs no Python:
 *   rank 0: fm_comm_unique_id(id)  -> ship the 128 bytes to every rank (any transport)
 *   all   : fm_comm_init(e, id, rank, world)
 * fm_comm_size returns the rank count (0 = no communicator).  Without a communicator (or with a
 * world of 1) the fm_fedavg_* calls compute the single-client result locally. */
#define FM_COMM_ID_BYTES 128
/* Local, non-collective: load librccl and resolve its entry points.  fm_comm_init is a collective (ncclCommInitRank
 * blocks until every rank has entered it), so call this on every rank first and agree on the result over the
 * transport that ships the id: a rank whose RCCL cannot be loaded must not leave its peers waiting inside the init. */
int fm_comm_preflight(void);
int fm_comm_unique_id(uint8_t* id128);
int fm_comm_init(fm_engine* e, const uint8_t* id128, int32_t rank, int32_t world);
int fm_comm_destroy(fm_engine* e);
int fm_comm_size(fm_engine* e);
/* FedAvg: state <- sum_ranks w_rank * state_rank, w_rank = n_rank / sum(n): the pre-scale kernel,
 * ONE in-place all-reduce of the whole fp32 state arena (44.8 MB for ResNet-18) and the float64
 * weighted mean of the num_batches_tracked counters (truncated on load like utils/FedAvg.py:13). */
int fm_fedavg_allreduce(fm_engine* e, float w);
/* FedAvg_tao over ranks: out[c] = sum_r t_r[c] n_r m_r[c] / sum_r n_r m_r[c] with m_r = this
 * rank's negative_mask (1 = class c is missing on this client; a rank that stands for several folded
 * clients passes n_i = 1 and their summed sample counts as the mask); 1.0 where no rank has it (:66-67). */
int fm_fedavg_tao(fm_engine* e, const double* t_host, double n_i, const float* negative_mask_host,
                  double* out_host);
/* FedAvg_proto over ranks: rows 2c, 2c+1 averaged over the ranks whose active_mask[c] = 1,
 * NaN rows where no rank annotates c (0/0 like :85-86).  proto/out: host [2C*D] fp32. */
int fm_fedavg_proto(fm_engine* e, const float* proto_host, double n_i, const float* active_mask_host,
                    float* out_host);

/* glob_model = deepcopy(net) at round start (utils/local_training.py:909, 1017):
 * snapshot the current state as the frozen eval-mode teacher. */
int fm_teacher_snapshot(fm_engine* e);
/* A fresh torch.optim.Adam every round (utils/local_training.py:912-913):
 * zero both moments and the step count.  One handle holds ONE optimizer's state (two NP-float arenas and a step count,
 * whichever optimizer steps): fm_adam_reset and fm_sgd_reset clear the same things. */
int fm_adam_reset(fm_engine* e, const fm_adam* hp);

/* ---- net(x) in eval mode: -> (feature[B,D], logits[B,C]) ----------------- */
/* utils/local_training.py:983, 1030, 1227 (student) / :944-947 (teacher).
 * use_teacher != 0 runs the snapshot taken by fm_teacher_snapshot. */
int fm_forward_eval(fm_engine* e, const float* x_dev, int32_t B, int32_t use_teacher,
                    float* feat_dev, float* logits_dev);

/* ---- training steps: forward + loss + backward + Adam.step --------------- */
/* Every step writes its scalar loss to *loss_dev (a device float the caller
 * reads back once per round instead of loss.item() every step) and bumps the
 * BN counters like a train-mode forward does.  bs_norm is args.batch_size: the
 * reference normalises by it, not by the actual batch length B. */

/* LocalUpdate.train (utils/local_training.py:628-703):
 * sum(BCEWithLogits(pos_weight)(z, y)) / (bs_norm * C). pos_weight: host[C]. */
int fm_step_bce(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B,
                const float* pos_weight_host, int32_t bs_norm, float* loss_dev);

/* train_FedMLP stage 1 (utils/local_training.py:920-967): two views, frozen
 * teacher, BCE on the active classes + MSE-to-teacher on the missing classes.
 * active_mask: host[C] of 0/1 (1 = class annotated by this client). */
int fm_step_stage1(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev,
                   int32_t B, const float* active_mask_host, int32_t annotation_num,
                   int32_t bs_norm, float* loss_dev);

/* train_FedMLP stage 2 (utils/local_training.py:1171-1192): masked BCE,
 * sup_cls = 1 - distill_cls (device [B,C]).  The reference's teacher forward
 * there is dead code and is not executed. */
int fm_step_stage2(fm_engine* e, const float* x_dev, const float* y_dev,
                   const float* distill_dev, int32_t B, float* loss_dev);

/* train_FixMatch (utils/local_training.py:789-818): weak/strong consistency.
 * pos_weight / pos_weight_unknown: host[C]. */
int fm_step_fixmatch(fm_engine* e, const float* xw_dev, const float* xs_dev, const float* y_dev,
                     int32_t B, const float* pos_weight_host, const float* pos_weight_unk_host,
                     const float* active_mask_host, int32_t annotation_num, int32_t bs_norm,
                     float* loss_dev);

/* ---- FedLSR and FedIRM (utils/local_training.py:1270-1326, 344-464) ---------
 * Three loss heads on TWO-VIEW logits z_dev [2B][C] (view 1 rows, then view 2 rows: fm_forward_train's layout), y_dev [B][C].
 * Each is one launch on the engine's stream with no synchronisation, writes every element of dz_dev [2B][C] and the scalar
 * *loss_dev, uses no atomics and gives the same bits from run to run; usable between fm_forward_train and fm_backward_step.
 *
 * fm_loss_fedlsr (:1294-1314): s_v = sigmoid(z_v), p = mix1 s_1 + (1 - mix1) s_2, pred_mix = sigmoid(2 log(p / (1 - p)));
 *   loss = mean over the B C elements of BCEWithLogits(pos_weight)(pred_mix, y) -- the reference feeds the probability in as
 *   a logit, and so does this -- + beta JS(q_1, q_2), q_v = clamp(sigmoid(3 z_v), 1e-6, 1), JS of :1258-1266 with
 *   KLDivLoss(reduction='mean'), i.e. the mean over all B C elements.  The means are over the actual B.  The clamp passes no
 *   gradient where it binds.  mix1 in [0, 1] is the caller's draw (np.random.beta(1, 1), one per step); beta is 0.4, or
 *   0.4 rnd / t_w while rnd < t_w.
 *   The one deviation: pred_mix is formed as p^2 / (p^2 + (1 - p)^2) with 1 - p = mix1 sigmoid(-z_1) + (1 - mix1) sigmoid(-z_2).
 *   torch's fp32 autograd of the logarithm returns NaN once p rounds to 1 (0 * inf); this form stays finite there and its
 *   derivative tends to 0.
 * fm_loss_fedirm_sup (:370-376): sum over both views and the active classes of BCEWithLogits(pos_weight)(z_v, y) /
 *   (bs_norm annotation_num).  rel_acc_dev [C][C] (NULL = skipped) += get_confuse_matrix(z_1, y) (:73-81): row i is
 *   sigmoid((sum_b z_1[b][:] y[b][i]) / (sum_b y[b][i] + 1e-8) / 2).  The reference hard-codes 8 classes there (range(8), tile 8);
 *   this is built for C and identical to the reference at C = 8.
 * fm_loss_fedirm_rel (:421-452): the supervised term + cw sum (sigmoid z_1 - sigmoid zt)^2 / bs_norm + cw kd(Q, target), where
 *   zt_dev [B][C] is the EMA model's logits on view 2 (no gradient), target_dev [C][C] the aggregated relation matrix,
 *   kd the symmetric kl_div(..., 'batchmean') of :109-113, Q = get_confuse_matrix(z_1[sel], sigmoid(z_1)[sel] > 0.5) over the rows
 *   whose every probability is > 0.7 or < 0.3 and whose uncertainty (:426-427) is < 2.  The selection and the pseudo-labels
 *   carry no gradient; kd's gradient reaches z_1 through Q.  With no row selected Q is the constant 0.5 matrix and kd has no
 *   gradient: decided on the device, no host read.  rel_acc_dev as above (NULL = skipped).  B <= 2048.
 * fm_step_fedlsr: the fused step like fm_step_fixmatch: two-view train-mode forward (BN statistics per view, running
 *   statistics updated view 1 then view 2), fm_loss_fedlsr's head, backward, Adam.  FM_ERR_ARG under a requires_grad mask.
 * FedIRM runs on the split step: fm_forward_train(x1, x2) -> fm_loss_fedirm_* -> fm_backward_step(dz). */
int fm_loss_fedlsr(fm_engine* e, const float* z_dev, const float* y_dev, const float* pos_weight_host, float mix1, float beta,
                   int32_t B, float* dz_dev, float* loss_dev);
int fm_loss_fedirm_sup(fm_engine* e, const float* z_dev, const float* y_dev, const float* pos_weight_host,
                       const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, int32_t B, float* rel_acc_dev,
                       float* dz_dev, float* loss_dev);
int fm_loss_fedirm_rel(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* pos_weight_host,
                       const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, float cw, const float* target_dev,
                       int32_t B, float* rel_acc_dev, float* dz_dev, float* loss_dev);
int fm_step_fedlsr(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev, int32_t B,
                   const float* pos_weight_host, float mix1, float beta, float* loss_dev);

/* ---- RSCFed, FedNoRo and CBAFed (utils/local_training.py:705-769, 115-234, 236-342) ---------
 * Three loss heads on SINGLE-VIEW logits z_dev [B][C], y_dev [B][C], with fm_loss_fedirm_sup's conventions: one launch on the
 * engine's stream, no synchronisation, no atomics, the same bits from run to run; every element of dz_dev [B][C] is written
 * (exact zeros where an element is not in the loss) and the scalar *loss_dev.  Value and gradient are formed in double from the
 * fp32 logits and rounded once.  There must be at least one active and one missing class (FM_ERR_ARG otherwise: torch forms
 * 0/0 or the mean of an empty tensor there), and bs_norm annotation_num < 2^24.
 *
 * fm_loss_rscfed (:719, 740-743): sum over the active classes of BCEWithLogits(pos_weight)(z, y) / (bs_norm annotation_num)
 *   + the mean over the actual B |missing| elements of (sigmoid z - sigmoid zt)^2.  zt_dev [B][C] (the EMA teacher's logits
 *   of view 2) gets no gradient.
 * fm_loss_lakd (LA_KD.forward, utils/FedNoRo.py:35-38, with train_FedNoRo's soft target): p = sigmoid(z),
 *   soft = sigmoid(zt / 0.8f); (1 - w_kd) sum_active BCE(p, y) / (B |active|) + w_kd sum_missing (p - soft)^2 / (B |missing|),
 *   the log clamped at -100 and binary_cross_entropy's backward (divisor max(p (1 - p), 1e-12)); both divisors use the actual B.
 *   Because p is formed in double, the clamp binds where sigmoid(z) rounds to 1 in double (|z| > 36.7), not in fp32 (|z| > 16.6).
 * fm_loss_cbafed (:247-269 warm-up, :303-333 stage 2): pos_weight_dev is a DEVICE vector [C], the client's loss_w, owned by the
 *   caller (one handle serves several clients).
 *   tao_host NULL (warm-up): the active-class BCEWithLogits(pos_weight) / (bs_norm annotation_num); pos_weight_dev is only
 *   read, counts_dev is not touched (may be NULL).
 *   tao_host [C] (stage 2): every decision of :303-316 is made on the device.  Per missing class i: hi = sigmoid(z) > tao[i],
 *   lo = sigmoid(z) < 1.f - tao[i] (fp32 compares), noise = #hi, clean = #lo; the label is 1 where hi (in registers: y_dev is
 *   not written); pos_weight_dev[i] = noise == 0 ? 1 : (float)((double)(noise + clean) / noise), written BEFORE the loss terms
 *   are formed (the reference rebuilds its criterion after the loop); with n_i = #(hi or lo) > 0 the class adds the sum over
 *   those rows of l[row][i] / n_i.  The active term is the warm-up's.  counts_dev int64 [C + 1] is ADDED to: n_i per missing
 *   class, B per active class, and sum n_i + B annotation_num in counts[C] (class_num_list and data_num of :312-320).
 * The fused steps return FM_ERR_ARG under a requires_grad mask, and give the bits of the split sequence
 * fm_forward_eval(teacher) / fm_forward_train -> fm_loss_* -> fm_backward_step (-> fm_teacher_axpby):
 * fm_step_rscfed: eval forward of x2 through the teacher slot (side lane where the engine has one), train forward of x1,
 *   fm_loss_rscfed, backward, Adam, then fm_teacher_axpby(w_teacher, w_student) over every state entry, reading the post-Adam
 *   student.  The next step's teacher forward sees the blended teacher.  With two lanes both views share the input staging:
 *   2 B <= max_images there, else the step runs on one lane.
 * fm_step_fednoro: teacher-slot eval forward and student train forward of the same x, fm_loss_lakd, backward, Adam.
 * fm_step_cbafed: one-view train forward, fm_loss_cbafed, backward, Adam; no host read. */
int fm_loss_rscfed(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* pos_weight_host,
                   const float* active_mask_host, int32_t annotation_num, int32_t bs_norm, int32_t B, float* dz_dev, float* loss_dev);
int fm_loss_lakd(fm_engine* e, const float* z_dev, const float* zt_dev, const float* y_dev, const float* active_mask_host, float w_kd,
                 int32_t B, float* dz_dev, float* loss_dev);
int fm_loss_cbafed(fm_engine* e, const float* z_dev, const float* y_dev, const float* active_mask_host, int32_t annotation_num,
                   int32_t bs_norm, const float* tao_host, int32_t B, float* pos_weight_dev, int64_t* counts_dev, float* dz_dev,
                   float* loss_dev);
int fm_step_rscfed(fm_engine* e, const float* x1_dev, const float* x2_dev, const float* y_dev, int32_t B,
                   const float* pos_weight_host, const float* active_mask_host, int32_t annotation_num, int32_t bs_norm,
                   float w_teacher, float w_student, float* loss_dev);
int fm_step_fednoro(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B, const float* active_mask_host, float w_kd,
                    float* loss_dev);
int fm_step_cbafed(fm_engine* e, const float* x_dev, const float* y_dev, int32_t B, const float* active_mask_host,
                   int32_t annotation_num, int32_t bs_norm, const float* tao_host, float* pos_weight_dev, int64_t* counts_dev,
                   float* loss_dev);

/* The RoFL client's head and fused step: include/fedmlp_hip_rofl.h. */

/* ---- prototype + t pass (utils/local_training.py:971-1002, 1208-1250) ---- */
/* Accumulators live in the engine: proto sums [2C,D], counts [2C], t counts [C]. */
int fm_proto_reset(fm_engine* e);
/* One eval batch: feature[B,D], logits[B,C], labels[B,C] on device.
 * active_mask / negative_mask: host[C] 0/1 (classes for prototypes / for t). */
int fm_proto_accumulate(fm_engine* e, const float* feat_dev, const float* logits_dev,
                        const float* labels_dev, int32_t B, const float* active_mask_host,
                        const float* negative_mask_host, float L, float U);
/* proto rows /= counts (zero_guard: leave a row with count 0 as is, the stage-2
 * variant :1240-1248; otherwise 0/0 = NaN like :997-999), t = counts / n_local.
 * Outputs on host: proto[2C*D] fp32, t[C] f64. */
int fm_proto_finalize(fm_engine* e, int32_t zero_guard, int64_t n_local,
                      const float* active_mask_host, float* proto_host, double* t_host);

/* ---- cosine tagging (CosineSimilarityFast, utils/local_training.py:1417-1435,
 *      call site :1052-1057) ------------------------------------------------ */
/* sim[k][n] = cos(f[n], P[2c_k]) - cos(f[n], P[2c_k+1]) for the n_cls classes
 * listed in classes_host.  feat_dev [N,D], proto_dev [2C,D], sim_dev [n_cls,N]. */
int fm_cos_tag(fm_engine* e, const float* feat_dev, int64_t N, const float* proto_dev,
               const int32_t* classes_host, int32_t n_cls, float* sim_dev);
/* Stable top-/bottom-k positions of one similarity row (utils/utils.py:24-35 via
 * utils/local_training.py:1061-1075): n_clean = #(sim>=0), n_noise = #(sim<0),
 * k_top = (int)(clean_thr*n_clean), k_bot = (int)(noise_thr*n_noise); writes the
 * positions of the k_top largest (descending, first position wins ties) and the
 * k_bot smallest (ascending) values to host arrays of capacity cap.
 * NaN: a NaN element counts as neither >= 0 nor < 0, is NEVER selected and is ranked nowhere -- the picks are those of the
 * row with its NaN elements removed, mapped back to positions (the reference's sorted() has no defined answer on NaN keys;
 * an all-zero feature row makes a NaN in every class).  -0.0 counts as >= 0 and ties with +0.0.  Thresholds are meant to
 * lie in [0, 1]; entries of top_host / bot_host beyond n_top / n_bot are not written. */
int fm_select_topk(fm_engine* e, const float* sim_dev, int64_t N, double clean_thr,
                   double noise_thr, int32_t cap, int32_t* top_host, int32_t* n_top,
                   int32_t* bot_host, int32_t* n_bot);
/* The same selection for EVERY missing class of a round (the loop of utils/local_training.py:1052-1112) in one launch pair
 * and one device-to-host read.  sim_dev [n_cls][N] (fm_cos_tag's output); class k's pool = the pool_n_host[k] positions
 * pool_rows_host[k*stride ..] of its similarity row, in pool order (find_indices_in_a, :901-902; ties go to the earlier pool
 * position), or all N rows when pool_rows_host is NULL.  Writes pool POSITIONS: top_host / bot_host [n_cls][cap],
 * n_top / n_bot [n_cls].  NaN elements of a pool are left out exactly as in fm_select_topk: never selected, ranked nowhere; a
 * fully-NaN class selects nothing. */
int fm_select_topk_rows(fm_engine* e, const float* sim_dev, int64_t N, int32_t n_cls, const int32_t* pool_rows_host,
                        const int32_t* pool_n_host, int32_t stride, double clean_thr, double noise_thr, int32_t cap,
                        int32_t* top_host, int32_t* n_top, int32_t* bot_host, int32_t* n_bot);

/* ---- HBM-resident input pipeline --------------------------- */
/* Train transform of dataset/dataset.py:40-53 on a uint8 cache of already-resized images
 * [N,3,H,W] kept in HBM: RandomAffine(10 deg, translate 2 %) with NEAREST sampling and fill 0,
 * RandomHorizontalFlip, ToTensor (/255), Normalize(mean, std).  The random draws are the
 * caller's.  params_dev[b] = int32 {c0, c1, c2, c3, c4, c5, flip (0/1), unused}: the inverse affine
 * matrix (PIL AFFINE convention: source = M * (x, y, 1)) in the 16.16 fixed point Pillow's
 * nearest-neighbour affine uses (libImaging/Geometry.c affine_fixed):
 *   c0, c1, c3, c4 = FIX(a0, a1, a3, a4), c2 = FIX(a2 + a0/2 + a1/2), c5 = FIX(a5 + a3/2 + a4/2),
 *   FIX(v) = floor(v * 65536 + 0.5); source pixel = ((c2 + c0 x + c1 y) >> 16, (c5 + c3 x + c4 y) >> 16).
 * Integer arithmetic: the result is bit-exact with the PIL pipeline (tests/golden/augment_pil.npz).
 * idx_dev[b] = sample index in the cache.  out_dev: fp32 NCHW [B,3,H,W], i.e. what fm_step_* consume.
 * mean/std: host[3]. */
int fm_augment(fm_engine* e, const uint8_t* cache_dev, const int32_t* idx_dev, const int32_t* params_dev,
               int32_t B, const float* mean_host, const float* std_host, float* out_dev);

/* The FixMatch strong view (dataset/dataset.py:63-77) on the same cache: the weak transform above (params_dev, the same
 * record and bits), then RandAugmentMC(n=2, m=10) of utils/FixMatch.py:205-219 -- two op slots, each skipped or one of the
 * 14 ops of its pool, applied to the uint8 result of the step before exactly as PIL chains them -- then CutoutAbs(16), /255,
 * Normalize.  Bit-exact with Pillow 12.2 (tests/golden/augment_strong_pil.npz).  The draws are the caller's; strong_dev[b] is
 * 20 int32 (80 bytes, 16-byte aligned per sample) holding everything that does not depend on pixels:
 *   [0..7]   slot 0: {op, p0, p1, p2, p3, p4, p5, 0}        [8..15]  slot 1, the same        [16..19] cutout {x0, y0, x1, y1}
 *   op: 0 AutoContrast, 1 Brightness, 2 Color, 3 Contrast, 4 Equalize, 5 Identity, 6 Posterize, 7 Rotate, 8 Sharpness, 9 ShearX,
 *       10 ShearY, 11 Solarize, 12 TranslateX, 13 TranslateY (the pool's order), 14 = slot skipped (its coin came up >= 0.5).
 *   p0 of Brightness / Color / Contrast / Sharpness: the blend factor v * 0.9 / 10 + 0.05 as fp32 bits;
 *   p0 of Posterize: the byte mask that keeps int(v * 4 / 10) + 4 bits; p0 of Solarize: the threshold 256 - int(v * 256 / 10);
 *   p0..p5 of Rotate / ShearX / ShearY / TranslateX / TranslateY: c0..c5 of the op's AFFINE matrix in the 16.16 form above, fill 0
 *       (Rotate: the matrix Image.rotate builds, cos / sin rounded to 15 places, about (W/2, H/2));
 *   cutout: the rectangle x0..x1, y0..y1 INCLUSIVE set to (127,127,127); x1 = W or y1 = H is clipped by the image.
 * Histograms, the Contrast mean and the AutoContrast / Equalize tables are computed on the device, on the image the step before
 * produced.  Five launches on the engine's stream whatever B and the ops, no host synchronisation.  The uint8 workspace
 * (max_images x (2 x 3 x H x W + 784) bytes) belongs to the handle and is allocated on the first call.  B <= max_images, W % 4 == 0. */
int fm_augment_strong(fm_engine* e, const uint8_t* cache_dev, const int32_t* idx_dev, const int32_t* params_dev,
                      const int32_t* strong_dev, int32_t B, const float* mean_host, const float* std_host, float* out_dev);

/* ---- evaluation metrics on the device ----------------------------------------------------- */
/* globaltest's metrics (utils/evaluations.py:41-66, utils/multilabel_metrixs.py) on device tensors.
 * scores_dev, labels_dev: fp32 [N][C] row-major, contiguous; a label is positive iff != 0.
 * ap_dev[C], auc_dev[C]: fp64; counts_dev[C][4]: int64 {tp, npos, npred, tn} with pred = score > threshold.
 * Any output pointer may be NULL (that part is skipped).  Enqueued on the engine's stream, no host
 * synchronisation, no atomics, bit-identical from run to run.  1 <= C <= FM_MAX_CLASSES, 1 <= N <= 2^22.
 * Workspace belongs to the handle and grows on demand (like fm_augment_strong's).
 * Per class, with P positives and Nn = N - P negatives, and IEEE fp32 compares on the scores:
 *   AP  = ( sum over positives i of (double)#{j positive : s_j >= s_i} / (double)#{j : s_j >= s_i} ) / P
 *   AUC = (double)( sum over positives i of 2 #{j negative : s_j < s_i} + #{j negative : s_j == s_i} ) / (2.0 P Nn)
 * which are sklearn's average_precision_score and auc(roc_curve(...)) with every tie grouped.  P = 0: AP = AUC = NaN;
 * Nn = 0: AUC = NaN, AP = 1 (fedmlp_amd/evaluations.py's host functions).  NaN scores are outside the contract. */
int fm_eval_metrics(fm_engine* e, const float* scores_dev, const float* labels_dev, int64_t N, int32_t C,
                    float threshold, double* ap_dev, double* auc_dev, int64_t* counts_dev);

/* ---- generic train step (the other baselines of main.py's --exp switch) -----
 * train_RSCFed (utils/local_training.py:705-769), train_FedNoRo (:115-234) and train_CBAFed
 * (:236-342) differ from the steps above only in the loss head on the [B,C] logits.  The split
 * step lets the host mirror compute that head: fm_forward_train runs the train-mode forward of one
 * view (x2_dev NULL) or two views (BN statistics per view, logits view-major [views*B][C]);
 * fm_backward_step takes d(loss)/d(logits) of the same shape, runs the backward pass and
 * optimizer.step().  The pair must be called back to back. */
int fm_forward_train(fm_engine* e, const float* x1_dev, const float* x2_dev, int32_t B, float* feat_dev,
                     float* logits_dev);
int fm_backward_step(fm_engine* e, const float* dlogits_dev);

/* ---- autograd path: train-mode net(x) -> loss.backward() -> optimizer.step() ------------------
 * Any loss computed by the caller (utils/local_training.py:370-379, 421-455, 520-551, 1294-1319 and a
 * user's own): the backward is split from the optimizer step by a gradient ACCUMULATOR owned by the
 * handle (NP floats, allocated on first use; the fused steps and fm_debug_get_grads never touch it).
 * fm_backward_grads: backward of the pending fm_forward_train / fm_forward_recompute (one or two views)
 *   from d(loss)/d(logits) [views*B][C] and d(loss)/d(feature) [views*B][D] (either may be NULL =
 *   zero); the parameter gradients are ADDED to the accumulator (the first backward after
 *   fm_zero_grad copies them: the same bits as the fused path's gradients); no optimizer step.
 *   Clears the pending forward.
 * fm_backward_grads_x: the same call plus d(loss)/d(image) of the pending forward's views: dx1_dev /
 *   dx2_dev fp32 [B][3][H][W] like the images fm_forward_train took (NULL = that view's gradient is not
 *   wanted; dx2_dev must be NULL after a one-view forward).  Each is WRITTEN, not added to, and is
 *   complete when the call's work on the engine's stream is.  The parameter gradients are bit-identical
 *   with and without it; without a dx pointer nothing is launched or allocated beyond
 *   fm_backward_grads (which is this call with both NULL).  fp32-class arithmetic in either precision.
 * fm_forward_recompute: the train-mode forward again, so that its saved activations exist for a
 *   following fm_backward_grads (the engine is deterministic: bit-identical saved tensors); BN
 *   running statistics and num_batches_tracked are NOT updated, nothing is written out.
 * fm_zero_grad: empties the accumulator.
 * fm_adam_step: torch.optim.Adam (coupled L2) over the accumulator with the handle's moments and step
 *   count (fm_adam_reset zeroes them); hp is read on every call.  An empty accumulator is skipped
 *   like torch skips parameters whose .grad is None.
 * fm_get_grads: the accumulator in state_dict order (conv weights OIHW; BN running statistics as
 *   zeros; fm_state_sizes' n_f32 floats) into a device buffer, enqueued without synchronising.
 * fm_bn_freeze: a handle flag (default 0) that fm_forward_train and fm_forward_recompute read.  While it is set
 *   every BatchNorm of those forwards applies its RUNNING statistics (mean = running_mean, istd =
 *   1/sqrt(running_var + eps)) instead of the batch's: running_mean / running_var and num_batches_tracked are
 *   not touched, and no image's output depends on the rest of the batch.  The pending forward remembers the
 *   mode it ran in: fm_backward_grads(_x) / fm_backward_step run the matching backward (dy = gamma istd dz
 *   through every BatchNorm; dgamma / dbeta against the running statistics, torch's eval-mode BatchNorm
 *   gradients) whatever the flag is by then.  Drop-connect / dropout multipliers apply as installed: freezing
 *   BatchNorm is not eval mode.  The fused fm_step_* ignore the flag: they always use batch statistics.
 * fm_bn_frozen: the flag (0 / 1). */
int fm_bn_freeze(fm_engine* e, int32_t on);
int fm_bn_frozen(fm_engine* e);
int fm_backward_grads(fm_engine* e, const float* dlogits_dev, const float* dfeat_dev);
int fm_backward_grads_x(fm_engine* e, const float* dlogits_dev, const float* dfeat_dev, float* dx1_dev, float* dx2_dev);
int fm_forward_recompute(fm_engine* e, const float* x1_dev, const float* x2_dev, int32_t B);
int fm_zero_grad(fm_engine* e);
int fm_adam_step(fm_engine* e, const fm_adam* hp);
int fm_get_grads(fm_engine* e, float* dev_out);
/* ---- more optimizers, gradient clipping and optimizer state for the autograd path ------------------
 * Kernels over the same arenas as fm_adam_step (weights, accumulator, the handle's two moment arenas), enqueued on the
 * engine's stream without synchronising.  The step functions behave like fm_adam_step: hp is read on every call, an empty
 * accumulator is skipped, and the handle's step count goes up by one.  The fused steps are not affected by any of them.
 * fm_sgd_reset: zero the moment arenas and the step count (what fm_adam_reset does; hp is validated, not kept).
 * fm_sgd_step: torch.optim.SGD's single-tensor update: g += weight_decay p; with momentum != 0, buf = g on the first step
 *   after a reset (no dampening, as torch), else buf = momentum buf + (1 - dampening) g; g = nesterov ? g + momentum buf :
 *   buf; p -= lr g.  buf is the first moment arena; momentum == 0 neither reads nor writes it.
 * fm_adamw_step: torch.optim.AdamW: p *= 1 - lr weight_decay, then Adam's update with no L2 folded into g.
 * fm_grad_norm: the L2 norm of the accumulator as ONE float written to norm_dev (device); two launches, no atomics: the
 *   same gradients give the same bits.  0 for an empty accumulator.  The engine's layout padding holds zeros and does not
 *   enter.
 * fm_clip_grad_norm: torch.nn.utils.clip_grad_norm_ (norm_type 2): accumulator *= min(1, max_norm / (norm + 1e-6)), the
 *   coefficient formed in fp32 on the device; the multiply always happens and a non-finite norm propagates.  norm_dev
 *   (device, may be NULL) receives the norm BEFORE clipping.  An empty accumulator: norm 0, nothing else.
 * fm_clip_grad_value: accumulator = clamp(accumulator, -clip, clip).
 * fm_optim_get_state / fm_optim_set_state: the two moment arenas in fm_get_grads' layout (state_dict order, conv weights
 *   OIHW, fm_state_sizes' n_f32 floats, zeros at the BN running statistics) to / from device buffers, and the step count.
 *   get: any pointer may be NULL.  set: the layout padding of the arenas is left zero; v_dev may be NULL (SGD: the second
 *   arena is zeroed); step >= 0, and step == 0 makes the next fm_sgd_step a first step.
 * Arguments: lr, weight_decay, momentum, eps, max_norm, clip >= 0; betas in [0, 1). */
int fm_sgd_reset(fm_engine* e, const fm_sgd* hp);
int fm_sgd_step(fm_engine* e, const fm_sgd* hp);
int fm_adamw_step(fm_engine* e, const fm_adam* hp);
int fm_grad_norm(fm_engine* e, float* norm_dev);
int fm_clip_grad_norm(fm_engine* e, float max_norm, float* norm_dev);
int fm_clip_grad_value(fm_engine* e, float clip);
int fm_optim_get_state(fm_engine* e, float* m_dev, float* v_dev, int64_t* step_host);
int fm_optim_set_state(fm_engine* e, const float* m_dev, const float* v_dev, int64_t step);
/* ---- per-layer requires_grad and optimizer parameter groups (autograd path) ------------------------------
 * One int32 per STATE ENTRY in reference key order (the order of fm_get_state / the state_dict: conv and linear weights,
 * biases, BatchNorm weight / bias / running_mean / running_var / num_batches_tracked); entries that are running
 * statistics or counters are buffers and their slots are ignored.  n_entries must be the entry count.
 * fm_set_trainable / fm_get_trainable: the requires_grad flag of every parameter (default: all ones).  The pending forward
 *   remembers the mask it ran under, like the BatchNorm mode.  Under a non-default mask fm_backward_grads(_x):
 *   - leave exact zeros at the frozen parameters' spans of the accumulator (copy and add form alike), and the same bits
 *     as an all-trainable backward at the trainable ones;
 *   - with no dx wanted, stop behind the first unit in forward order that has a trainable parameter (ResNet-18: stem,
 *     layer1.0 .. layer4.1, fc; EfficientNet-B0: stem, _blocks.0 .. _blocks.15, head, _fc): nothing of an earlier unit is
 *     enqueued, and head-only training is the classifier's backward alone;
 *   - do not launch a frozen convolution's weight gradient where it is a launch of its own.
 *   The fused fm_step_* and fm_backward_step train every layer: under a non-default mask they return FM_ERR_ARG.  With the
 *   default mask everything is launch for launch what it is without these calls.
 *   A frozen parameter still sees its BatchNorm running statistics move in a batch-statistics forward (torch's behaviour):
 *   fm_bn_freeze is the switch for that.
 * fm_optim_groups: the parameter group of every parameter, 0 .. n_groups - 1, or -1 = not optimized; n_groups <=
 *   FM_MAX_GROUPS; n_groups = 0 clears the table.
 * fm_adam_step_groups / fm_adamw_step_groups / fm_sgd_step_groups: fm_adam_step / fm_adamw_step / fm_sgd_step with hp[i] the
 *   hyper-parameters of group i (n = the table's group count): one launch over the parameters' entry table, the same
 *   arithmetic per element to the bit.  A parameter in no group or frozen is not touched: no update, no weight decay,
 *   moments as they were (torch: .grad is None).  One step count per handle, whatever the groups. */
#define FM_MAX_GROUPS 8
int fm_set_trainable(fm_engine* e, const int32_t* flags, int32_t n_entries);
int fm_get_trainable(fm_engine* e, int32_t* flags, int32_t n_entries);
int fm_optim_groups(fm_engine* e, const int32_t* group_of_entry, int32_t n_entries, int32_t n_groups);
int fm_adam_step_groups(fm_engine* e, const fm_adam* hp, int32_t n);
int fm_adamw_step_groups(fm_engine* e, const fm_adam* hp, int32_t n);
int fm_sgd_step_groups(fm_engine* e, const fm_sgd* hp, int32_t n);
/* teacher <- w_teacher*teacher + w_student*student over every state entry (train_RSCFed's EMA,
 * utils/local_training.py:751-759, weights 0.999 / 0.001). */
int fm_teacher_axpby(fm_engine* e, float w_teacher, float w_student);
/* teacher <- alpha*teacher + (1-alpha)*student over the PARAMETERS only (update_ema_variables,
 * utils/local_training.py:62-65; the caller forms alpha = min(1 - 1/(step+1), ema_decay)): BatchNorm running
 * statistics and num_batches_tracked of the teacher stay untouched.  Both weights are rounded to fp32 once. */
int fm_teacher_ema_params(fm_engine* e, double alpha);
/* exchange the student and teacher slots (so fm_set_state / fm_get_state reach the teacher) */
int fm_teacher_swap(fm_engine* e);

/* ---- EfficientNet-B0 training-time randomness -----------------------------------
 * The reference's model draws drop-connect (MBConvBlock, p = 0.2*idx/16 per block, per sample)
 * and dropout (p = 0.2 before `_fc`) inside net(images) (utils/local_training.py:657, 937-947,
 * 1178 through efficientnet_pytorch 0.7.1).  Here the draws are the caller's: device arrays of
 * MULTIPLIERS, kept by pointer until replaced (NULL = identity, i.e. no drop).
 *   drop_connect_dev [16][imgs]   imgs = images in the next train step (2B for two-view steps,
 *                                 view-major), value floor(keep+U)/keep
 *   dropout_dev      [imgs][1280] value 0 or 1/(1-p)
 * Ignored by model 0. */
int fm_set_stochastic(fm_engine* e, const float* drop_connect_dev, const float* dropout_dev);
/* feature width of the model: 512 (ResNet-18) or 1280 (EfficientNet-B0) */
int fm_feature_dim(fm_engine* e);
/* The stream mode that was actually set up (fm_config.reserved[1] asks; fm_create falls back to one stream when the
 * second activation / workspace set would not fit in free device memory): 0 teacher + weight gradients on the side
 * stream, 2 teacher only, 1 one stream. */
int fm_stream_mode(fm_engine* e);
/* How the fp32 convolution GEMMs (ResNet-18's 3x3 / 1x1 convs, EfficientNet's wide 1x1 convs) form their products right
 * now: 0 = v_mfma_f32_16x16x4_f32; 9 / 6 = each fp32 product as 9 / 6 exact bf16 partial products on
 * v_mfma_f32_16x16x32_bf16, accumulated in fp32 (csrc/split3.h).  fm_products(e): the form of this handle, set at
 * fm_create from fm_config.reserved[2].  fm_mfma_products(): what reserved[2] = 0 resolves to (6 in the shipped library;
 * the test-only environment variable FM_MFMA_SPLIT = 0 | 6 | 9 overrides it and is read once per fm_create, never per
 * launch).  The reference has one arithmetic (utils/local_training.py:14 imports autocast and never uses it); cuDNN picks
 * its own algorithm behind nn.Conv2d (model/all_models.py:53-54). */
int fm_mfma_products(void);
int fm_products(fm_engine* e);
/* 1 when the handle's conv GEMMs read their operands as bf16 planes written by the producing kernels (ResNet-18 in a split
 * product form: csrc/pconv.hip, pwgrad.hip, planes_ew.hip; activations between convs then exist only as planes), 0 when they
 * read fp32 tensors (csrc/igemm.hip, wgrad.hip: EfficientNet-B0, the fp32 matrix pipe, FM_PLANES=0).  Same arithmetic either way. */
int fm_planes_mode(fm_engine* e);

/* ---- measurement hooks (bench.py roofline leg) ---------------------------- */
/* When enabled, HIP events bracket every convolution GEMM launch on the
 * engine's stream; fm_profile_read drains them (synchronises) and returns, per
 * kernel (family 0 = igemm_kernel<128,128,2,0,...>, 1 = igemm_kernel<64,192,4,0,...>,
 * 2 = igemm_kernel<64,256,4,2,...> (7x7 stem): conv forward + data gradient; 3 = wgrad_kernel<128,128,2,4>,
 * 4 = wgrad_kernel<64,192,4,3> (64-channel 3x3 layers) and the skinny 1x1 wgrad, 5 = the 7x7 stem's weight
 * gradient), the launch count, total milliseconds and algorithmic FLOPs since the last read.  Planes mode (fm_planes_mode):
 * 0 / 1 = pconv_kernel<4 | 2, 4, 2, SP, true> (3x3 stride-1 convs and their data gradients, M >= 128 | M = 64), 6 / 7 =
 * pconv_kernel<4 | 2, 4, 2, SP, false> (stride-2 / 1x1 convs, parity classes), 3 / 4 = pwgrad_kernel<4 | 2, ...>,
 * 8 = pwgrad_ring_kernel<SP> (weight gradients of the 3x3 stride-1 convs on the 56 x 56 and 28 x 28 maps), 2 = stem_rows_kernel<SP>
 * (the 7x7 stem forward at 112-pixel output rows; other input sizes: igemm_kernel<64,256,4,2,...>). */
#define FM_PROFILE_FAMILIES 9
int fm_profile_enable(fm_engine* e, int32_t on);
int fm_profile_read(fm_engine* e, int32_t family, int64_t* launches, double* ms, double* flops);

/* Per-op timing of the EfficientNet-B0 graph (tools/op_profile.py): while enabled, HIP events bracket every op
 * of the step; a call drains them and, when buf != NULL, writes "op@block<TAB>calls<TAB>total ms" lines and
 * resets the table.  Blocks: -1 stem, 0..15 train forward, 100 head, 201..216 / 300 eval forward,
 * 399..415 / 500 backward. */
int fm_profile_ops(fm_engine* e, int32_t enable, char* buf, int32_t cap);

/* Kernel-level test hooks (fm_debug_*: single-kernel entry points, saved activations, last gradients) are declared in
 * fedmlp_hip_debug.h; they are not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* FEDMLP_HIP_H */
