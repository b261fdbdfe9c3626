"""NIC -- dense voxel encoder + LSTM decoder (BASELINE config 2).

Drop-in for ``AttemptFour/Model/NIC.py`` (class NIC, lines 19-325): same constructor
arguments (NIC.py:22), ``call`` (100-145), ``greedy_predict`` (148-195), ``train_step``
(198-252), ``test_step`` (254-299).  The step is a fixed sequence of HIP kernel launches
over static buffers (captured into a hipGraph after warm-up):

  forward : [dropout] -> split-K GEMM (B x N x E, bias+LeakyReLU) -> [dropout] -> BatchNorm
            -> embedding gather -> one GEMM for every timestep's input projection
            -> T+1 fused LSTM step kernels -> vocab GEMM -> fused softmax/CE/accuracy/dlogits
  backward: vocab dW/dX GEMMs -> T+1 fused LSTM backward steps -> dU, dW, dX GEMMs
            -> embedding scatter -> BatchNorm/LeakyReLU backward -> encoder dW GEMM
  update  : [all-reduce] -> per-variable norms -> clip + Adam over the flat arena.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import compat
from .arena import ParamArena
from .model_base import (ModelBase, Metrics, _r4, S_IN, S_FEAT, S_LSTM_IN, BN_EPS, BN_MOMENTUM, S_SS_COIN, S_SS_DRAW,
                         SS_MAX_POSITIONS, S_SCST_LAST, ScheduledSampling, SelfCritical, SemanticTarget, check_sampling, check_beam,
                         _TokenChoice, _BeamDecode, EncGram, EncUpdate, StepRoute)
from .evaluate import REWARD_KINDS, REWARD_MAX_LEN, REWARD_MAX_REFS, ROUGE_BETA, ROUGE_KIND, pack_references
from .lstm_layer import lstm_layer_step_fwd, lstm_layer_fwd, lstm_layer_bwd
from .ops import ACT_LEAKY, LIVE_ROWS_M, LIVE_ROWS_K, contrastive_work_floats

ENC_SPLITS = 16      # K splits of the streaming encoder forward: 16 column groups x 16 splits = one workgroup per CU


class NIC(ModelBase):
    BN = "batch_norm"       # the BatchNormalization layer that owns the moving statistics (fc_nic: its own)
    # ---- A/B switches of this model (ModelBase declares the shared ones; same rules)
    compact_head = True         # False: the vocabulary head over all T * B position-ordered rows; tests/test_gpu_compact_head.py
    stage_fwd = True            # False: batch staging and encoder forward as two launches; INTEGRATION.md 4, tests/test_gpu_stage_forward.py
    fuse_enc_update = True      # False: the encoder kernel's gradient is written and updated like any other; tests/test_host_nic.py
    fuse_tail = True            # False: the encoder tail (BatchNorm, Dropouts, LeakyReLU') as separate launches; tools/ab_bench.py
    fused_xproj = False         # True: the LSTM input projection on the one-round GEMM family (gemm_fused); tools/ab_fused.py
    fused_head_grads = False    # True: the head's dW + bias gradient on gemm_fused (with g3_riders = False); tools/ab_fused.py
    fused_lstm_grads = False    # True: the LSTM's parameter gradients on gemm_fused (with g3_riders = False); tools/ab_fused.py
    side_head = True            # False: the head's dW stays on the main stream under use_side_streams; tools/side_bench.py
    SUPPORTS_INPUT_CORRUPTION = True    # scan_dropout= / word_dropout= (ModelBase._stage_batch(corrupt=True))
    SUPPORTS_GRAD_ACCUMULATION = True   # gradient_accumulation_steps= (ModelBase._train_step_accum)
    SUPPORTS_DISTILLATION = True        # CategoricalCrossentropy(distillation=) / set_teacher (ModelBase._teach)
    STEP_FEATURES = ("scheduled_sampling", "self_critical", "corruption", "semantic")   # what train_step checks (compat)

    def __init__(self, input_size, units, embedding_dim, vocab_size, max_length, dropout_input, dropout,
                 dropout_lstm, input_reg, lstm_reg, output_reg, norm="batch", scheduled_sampling=None, self_critical=None,
                 scan_dropout=None, word_dropout=None, semantic=None, **kw):
        super().__init__(**kw)
        self.N, self.U, self.E, self.V, self.max_length = int(input_size), int(units), int(embedding_dim), int(vocab_size), int(max_length)
        self.r_in, self.r_feat, self.r_lstm = float(dropout_input), float(dropout), float(dropout_lstm)
        # NIC.py:53-55: the output layer is regularised with lstm_reg (quirk kept)
        self.l2_in, self.l2_lstm, self.l2_out = float(input_reg), float(lstm_reg), float(lstm_reg)
        assert norm in ("batch", "layer")
        self.norm = norm
        if self.U % 16:
            raise ValueError("units must be a multiple of 16 (LSTM step kernel tile)")
        N, U, E, V = self.N, self.U, self.E, self.V
        # scheduled_sampling (model_base.ScheduledSampling): train_step feeds each caption row the model's own token with
        # the schedule's probability (tnt_scheduled_feedback_f32); None keeps the teacher-forced step
        if scheduled_sampling is not None:
            if not isinstance(scheduled_sampling, ScheduledSampling):
                raise ValueError("scheduled_sampling must be None or a model_base.ScheduledSampling, got "
                                 f"{scheduled_sampling!r}")
            if E % 4 or E > 1016:
                raise ValueError(f"scheduled sampling needs embedding_dim % 4 == 0 and <= 1016 "
                                 f"(tnt_scheduled_feedback_f32), got {E}")
        self.scheduled_sampling = scheduled_sampling
        # self_critical (model_base.SelfCritical): train_step runs the self-critical step (train_step_scst); its rollout is
        # the scheduled-sampling forward at a constant p = 1 in sample mode
        if self_critical is not None:
            if not isinstance(self_critical, SelfCritical):
                raise ValueError(f"self_critical must be None or a model_base.SelfCritical, got {self_critical!r}")
            if E % 4 or E > 1016:
                raise ValueError(f"self-critical training needs embedding_dim % 4 == 0 and <= 1016 "
                                 f"(tnt_scheduled_feedback_f32), got {E}")
            if self_critical.end_id >= V:
                raise ValueError(f"self-critical end_id {self_critical.end_id} is not below vocab_size {V}")
            if self_critical.score_on == "device" and self_critical.reward != ROUGE_KIND and V > 65536:
                raise ValueError(f"self-critical score_on='device' packs 16 bits per token id (evaluate.RewardTable): "
                                 f"vocab_size {V} is above 65536")
        self.self_critical = self_critical
        self._rollout_ss = ScheduledSampling.linear(1.0, 0.0, 1.0, mode="sample") if self_critical is not None else None
        # semantic (model_base.SemanticTarget): train_step adds weight * mean_b (1 - cos(x_b W + bias, guse_b)) to its loss, x_b
        # the feature row the first LSTM step receives and guse the batch's fifth input; one layer of its own (guse_out), whose
        # arena entries sit behind every other; None builds nothing and keeps launches and bits
        if semantic is not None and not isinstance(semantic, SemanticTarget):
            raise ValueError(f"semantic must be None or a model_base.SemanticTarget, got {semantic!r}")
        self.semantic = semantic
        compat.check(self, ("scheduled_sampling", "self_critical", "semantic"))
        self.ldx, self.ldV = _r4(N), _r4(V)
        self.layers_spec = OrderedDict([
            ("dense_img", ["kernel", "bias"]),
            ("batch_norm", ["gamma", "beta", "moving_mean", "moving_variance"]),
            ("emb_text", ["embeddings"]),
            ("lstm", ["kernel", "recurrent_kernel", "bias"]),
            ("time_distributed_softmax", ["kernel", "bias"])])
        self.keras_shapes = OrderedDict([
            ("dense_img/kernel", (N, E)), ("dense_img/bias", (E,)),
            ("batch_norm/gamma", (E,)), ("batch_norm/beta", (E,)),
            ("batch_norm/moving_mean", (E,)), ("batch_norm/moving_variance", (E,)),
            ("emb_text/embeddings", (V, E)),
            ("lstm/kernel", (E, 4 * U)), ("lstm/recurrent_kernel", (U, 4 * U)), ("lstm/bias", (4 * U,)),
            ("time_distributed_softmax/kernel", (U, V)), ("time_distributed_softmax/bias", (V,))])
        if semantic is not None:
            self.G, self.ldG = semantic.dim, _r4(semantic.dim)
            self.layers_spec[SemanticTarget.LAYER] = ["kernel", "bias"]
            self.keras_shapes["guse_out/kernel"], self.keras_shapes["guse_out/bias"] = (E, self.G), (self.G,)
        a = self.arena = ParamArena(self.device)
        a.add("dense_img/kernel", (N, E), self.l2_in)
        a.add("dense_img/bias", (E,))
        a.add("batch_norm/gamma", (E,))
        a.add("batch_norm/beta", (E,))
        a.add("emb_text/embeddings", (V, E))
        a.add("lstm/kernel", (E, U, 4), self.l2_lstm)
        a.add("lstm/recurrent_kernel", (U, U, 4))
        a.add("lstm/bias", (U, 4))
        a.add("time_distributed_softmax/kernel", (U, self.ldV), self.l2_out)
        a.add("time_distributed_softmax/bias", (self.ldV,))
        if semantic is not None:            # behind every entry of the model without it; rows padded as the head pads V
            a.add("guse_out/kernel", (E, self.ldG), semantic.reg)
            a.add("guse_out/bias", (self.ldG,))
        a.finalize()
        self.mov_mean, self.mov_var = self._f(E), torch.ones(E, dtype=torch.float32, device=self.device)
        self.drop_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        if scheduled_sampling is not None or self_critical is not None:     # the schedule's parameters, read by the kernel
            self.ss_sched = torch.tensor((scheduled_sampling or self._rollout_ss).params(), dtype=torch.float64,
                                         device=self.device)
        self._init_weights(np.random.default_rng(self.seed))
        self._shape = None
        self._init_step_state()
        # scan_dropout (model_base.ScanDropout) / word_dropout (model_base.WordDropout): train_step corrupts the staged batch
        # (tnt_input_corrupt_f32, one launch behind the staging); None or rate 0 issues nothing.  The setters validate
        self.scan_dropout, self.word_dropout = scan_dropout, word_dropout

    def _init_step_state(self):
        """what exists only once a step or a decode has asked for it (fc_nic.NICfc, which has its own constructor, too)"""
        self._enc_gram = None           # EncGram of the last training forward that left the Gram by-products (_forward)
        self._enc_last_fused = None     # (x, dpre, rows) of the last _bwd_enc that handed the encoder gradient to the update
        self._enc_grad_stale = None     # ... while the gradient buffer lags behind them (train_step; get_gradient forms it)
        self._enc_shard = None          # the row-sharded encoder update's spans and buffers (_enc_shard_state)
        self._head_live_est = None      # the head's live row count at the warm-up step (_head_plan_rows)
        self._plan_staged = {}          # step key -> whether its recording left the encoder forward to the staging launch
        self._scst = None               # the self-critical step's buffers (_scst_bufs)
        self._beam_bufs = {}            # beam_search's static buffers per (B, k, max_len, end_id[, G])

    # ------------------------------------------------------------------ weights
    def _init_weights(self, rng):
        """Initialisers of NIC.py:64-98 (GlorotNormal kernels, keras defaults elsewhere); values only
        matter for benchmarks -- parity tests inject weights."""
        N, U, E, V = self.N, self.U, self.E, self.V
        tn = lambda shape, std: np.clip(rng.standard_normal(shape), -2, 2) * std / 0.8796
        self.set_weight("dense_img/kernel", tn((N, E), np.sqrt(2.0 / (N + E))))
        self.set_weight("emb_text/embeddings", rng.uniform(-0.05, 0.05, (V, E)))
        lim = np.sqrt(6.0 / (E + 4 * U))
        self.set_weight("lstm/kernel", rng.uniform(-lim, lim, (E, 4 * U)))
        q = np.concatenate([np.linalg.qr(rng.standard_normal((U, U)))[0] for _ in range(4)], axis=1)
        self.set_weight("lstm/recurrent_kernel", q)
        b = np.zeros(4 * U); b[U:2 * U] = 1.0          # unit_forget_bias
        self.set_weight("lstm/bias", b)
        self.set_weight("time_distributed_softmax/kernel", tn((U, V), np.sqrt(2.0 / (U + V))))
        self.set_weight("batch_norm/gamma", np.ones(E))
        if self.semantic is not None:       # glorot_uniform, drawn behind every other weight: those keep their values
            lim = np.sqrt(6.0 / (E + self.G))
            self.set_weight("guse_out/kernel", rng.uniform(-lim, lim, (E, self.G)))

    def _state_map(self):
        return {f"{self.BN}/moving_mean": self.mov_mean, f"{self.BN}/moving_variance": self.mov_var}

    def get_gradient(self, name):
        """Last computed gradient of a trainable (keras layout, *without* the L2 term, which the
        optimizer kernels add on the fly)."""
        self._frozen_gradient_refuse(name)
        st = self._enc_grad_stale
        if name == "dense_img/kernel" and st is not None:
            # the fused step consumed X^T dpre inside the optimizer launches without writing it: its operands are still
            # in place, materialise it on request
            x, dpre, rows = st
            self.be.dense_dw_skinny(x, dpre, self.arena.g(name), self.N, self.E, rows, self.ldx)
            self._enc_grad_stale = None
        return super().get_gradient(name)

    def _enc_update_fused(self, rows, defer=None):
        """True when the encoder kernel's gradient is consumed inside the optimizer launches instead of being written
        out (tnt_dense_dw_sqnorm_f32 / tnt_dense_dw_adam_f32): the single-process fused step with Adam, no AGC.
        ``defer``: asked ahead of the step (_stage_fwd_args) -- whether that step will be the fused one."""
        opt = self.optimizer
        defer = self._tail.deferring if defer is None else defer
        # (a frozen encoder kernel has no update at all: with skip_frozen_work off its gradient is written like any other)
        return bool(defer and self.dp_world == 1 and self.fuse_enc_update and not self._frozen("dense_img/kernel")
                    and opt is not None and opt.kind == "adam" and not self.agc and rows <= 64
                    and self.E % 512 == 0
                    and self.arena.entries["dense_img/kernel"].seg == 0
                    # one norm-partial slot per workgroup inside the variable's own span slots
                    and min((self.N + 15) // 16, 256) * (self.E // 512) <= self.arena.spans.first_host[1])

    # ------------------------------------------------------------------ buffers
    def _build(self, B, T):
        if self._shape == (B, T):
            return
        f = self._f
        N, U, E, V, ldV = self.N, self.U, self.E, self.V, self.ldV
        R1 = (T + 1) * B
        self.x = f(B, self.ldx)
        self.xd = f(B, self.ldx) if self.r_in > 0 else self.x
        self.cap = torch.zeros(B, T, dtype=torch.int32, device=self.device)
        self.tgt = torch.zeros(T * B, dtype=torch.int32, device=self.device)
        self.enc_pre, self.enc_y = f(B, E), f(B, E)
        # K-split partials of the streaming encoder forward (tnt_dense_fwd_stream_f32); None -> generic split-K GEMM
        ok = self.norm == "batch" and B <= 256 and E % 32 == 0 and N % 4 == 0
        self.enc_part = f(ENC_SPLITS * B * E) if ok else None
        self.enc_gx = self.enc_w2 = None        # Gram by-products of the forward (allocated on first use, outside captures)
        self.enc_yd = f(B, E) if self.r_feat > 0 else self.enc_y
        self.xhat = f(B, E)
        self.inv_std = f(max(B, E))
        self.Xin = f(R1, E)
        self.Xin_d = f(R1, E) if self.r_lstm > 0 else self.Xin
        self.XZ = f(R1, U, 4)
        self.Hs, self.Cs = f(T + 2, B, U), f(T + 2, B, U)
        self.gates = f(T + 1, B, U, 4)
        self.Out = f(T, B, U)
        self._init_seq_lstm(B, U)        # persistent sequence kernel: opt-in per shape and per device
        self.logits = f(T * B, ldV)
        self.loss_row, self.corr_row = f(T * B), f(T * B)
        # row map of the vocabulary head (compact_head; tnt_stage_batch_map_f32): compacted row of every (t, b) or -1, the
        # rows' multiplicities and targets, and the number of rows
        self.head_pos = torch.full((T * B,), -1, dtype=torch.int32, device=self.device)
        self.head_w = f(T * B)
        self.head_tgt = torch.zeros(T * B, dtype=torch.int32, device=self.device)
        self.head_live = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._head_live_est = None
        self.met = f(8)
        self.dOut = f(T * B, U)
        self.dZ = f(R1, U, 4)
        self.da_pass, self.dc, self.dout = f(B, U), f(B, U), f(B, U)
        self.dXin = f(R1, E)
        self.dyd, self.dpre = f(B, E), f(B, E)
        be = self.be
        self._alloc_splitk([(B, E, N), (T * B, U, V), (R1, E, 4 * U), (R1, 4 * U, E), (T * B, V, U)])
        nch = max(be.bn_nchunk(B), be.bn_nchunk(R1), be.bn_nchunk(T * B))
        self.work = f(max(E, 4 * U, ldV) * (2 * nch + 1))
        self.work2 = f(max(E, 4 * U, ldV) * (2 * nch + 1))
        self.rowsq = f(B * T)
        if self.semantic is not None:       # the staged target, the prediction (its gradient in place), the rows' loss and cos
            self.sem_g, self.sem_z = f(B, self.ldG), f(B, self.ldG)
            self.sem_loss, self.sem_cos = f(B), f(B)
            if self.semantic.contrastive:   # the entry's scratch, the rows' hits and its two means (loss, top1)
                soft = self.semantic.soft_temperature is not None
                self.sem_work = f(contrastive_work_floats(B, soft))
                self.sem_hit = torch.zeros(B, dtype=torch.int32, device=self.device)
                self.sem_out = f(2)
        self.emb_seg = self.arena.entries["emb_text/embeddings"].seg
        self._shape = (B, T)
        self._graphs = {}
        if self.optimizer is not None and self.opt_m is None:
            self._init_optimizer_state()
        self.built = True

    def _stage_inputs(self, data):
        self._route = StepRoute()
        x, cap, a0, c0 = data[:4]           # (a fifth input, the sentence embedding, is train_step's / test_step's)
        cap_t = self._to_dev(cap, torch.int32)
        B, T = cap_t.shape
        self._build(B, T)
        xs = self._to_dev(x, torch.float32)
        assert xs.shape == (B, self.N), f"betas shape {tuple(xs.shape)} != {(B, self.N)}"
        self.x[:, :self.N].copy_(xs)
        self.cap.copy_(cap_t)
        self.Hs[0].copy_(self._to_dev(a0, torch.float32))
        self.Cs[0].copy_(self._to_dev(c0, torch.float32))
        return B, T

    def _head_map_bufs(self, B, T):
        """The vocabulary head over the DISTINCT rows only (``compact_head``, default on).  The text LSTM carries its output
        through the padded tail of a caption (fed id 0) and the targets there are all 0, so those positions repeat one row
        of Out, logits, loss and dlogits; the loss is not masked, so they count -- once, weighted by their multiplicity.
        Taken by train_step where the step is the persistent chains + the gemm3 products of one process and nothing else
        writes or reads the head's buffers by position: no scheduled sampling, self-critical step, AGC, label smoothing,
        unlikelihood (its candidates are a row's earlier positions, which the compacted rows have lost), token weights /
        focal loss / normalise="weights" (the weighted head has no row-multiplicity form), data parallel; a distilled step
        (train_step stages it with head_map=False: a distinct row has no teacher row to pair with).
        Everything else (test_step, decode, the per-step LSTM kernels, other backends) keeps the position-ordered
        buffers."""
        be = self.be
        ok = (self.compact_head and self._seq_lstm and self.seq_xch is not None
              and hasattr(be, "stage_batch_map") and hasattr(be, "softmax_cce_live") and hasattr(be, "gemm3")
              and self.use_gemm3 and self.g3_riders
              and not compat.any_on(self, ("dp", "scheduled_sampling", "self_critical", "agc", "label_smoothing",
                                           "unlikelihood", "token_weights"))
              and self.U % 4 == 0)
        if not ok:
            return None
        return (self.head_pos, self.head_w, self.head_tgt, self.head_live, self.loss_row, self.corr_row)

    def _gram_fwd(self, B, defer=None):
        """the training forward leaves X X^T and sum W^2 behind (tnt_dense_fwd_stream_gram_f32): the optimizer step takes the
        encoder kernel's gradient X^T dpre without writing it, and its clip-by-norm factor follows from these"""
        return (self._fused_tail(B) and self.enc_part is not None and self._enc_update_fused(B, defer)
                and self.N % 16 == 0 and self.E >= 512)

    def _gram_bufs(self):
        if self.enc_gx is None:
            self.enc_gx, self.enc_w2 = self._f(ENC_SPLITS * 64 * 64), self._f(ENC_SPLITS * (self.E // 32))

    def _stage_fwd_args(self, B):
        """``stage_fwd`` (default on): train_step's staging launch and the encoder forward are ONE launch
        (tnt_dense_fwd_stream_gram_stage_f32) where the step's first kernel is the Gram form of the streaming forward on
        the staged betas themselves (no input Dropout), and the step is the single-process fused one.  Everything else
        keeps the two launches."""
        ok = (self.stage_fwd and self.r_in == 0 and hasattr(self.be, "dense_fwd_stream_gram_stage")
              and self._gram_fwd(B, defer=bool(self.fused_update)))
        if not ok:
            return None
        self._gram_bufs()
        return (self.arena.p("dense_img/kernel"), self.enc_part, self.enc_gx, self.enc_w2, self.E, self.E, ENC_SPLITS)

    def _fused_tail(self, B):
        """one-launch encoder tail (tnt_enc_tail_*): BatchNorm encoder, batch <= 256 rows, E % 4 == 0"""
        return (self.norm == "batch" and B <= 256 and self.E % 4 == 0 and self.fuse_tail
                and not self._sync_bn_on())        # synchronised BatchNorm: the statistics leave the kernel for a collective

    # ------------------------------------------------------------------ sentence-embedding target (model_base.SemanticTarget)
    def _semantic_target(self, inputs):
        """the batch's fifth input as a (B, G) float32 tensor on the device, checked in front of every launch; None without
        semantic= (a fifth input is then ignored)"""
        if self.semantic is None:
            return None
        if len(inputs) < 5 or inputs[4] is None:
            raise ValueError(f"a model with semantic= takes (betas, cap, a0, c0, guse): the batch has {len(inputs)} inputs")
        B, G = int(np.shape(inputs[1])[0]), self.G
        if tuple(np.shape(inputs[4])) != (B, G):
            raise ValueError(f"guse shape {tuple(np.shape(inputs[4]))} != {(B, G)} (batch, SemanticTarget.dim)")
        return self._to_dev(inputs[4], torch.float32)

    def _semantic_key(self):
        """what a plan / graph key carries for the term: the cosine loss keeps ("semantic",)"""
        return ("semantic", "contrastive") if self.semantic.contrastive else ("semantic",)

    def _semantic_slots(self):
        """the term's metrics and their slots of ``met``"""
        if self.semantic is None:
            return {}
        if self.semantic.contrastive:
            return dict(semantic=SemanticTarget.SLOT, semantic_top1=SemanticTarget.TOP1_SLOT)
        return dict(semantic=SemanticTarget.SLOT)

    def _semantic_stage(self, guse):
        """the target into its static buffer (a copy in front of the step: a replayed plan or graph reads each batch's own)"""
        if guse is not None:
            self.sem_g[:, :self.G].copy_(guse)

    def _semantic_fwd(self, B, want_grad):
        """z = x W + bias on the model's product route, then tnt_cosine_loss_f32 (tnt_contrastive_loss_f32 under
        loss="contrastive", with semantic_top1 into met[5]): the rows' loss and cos, the unweighted mean
        into met[6] and (``want_grad``) the gradient of weight * mean in place of z.  x = xin[:B], the feature rows the first
        LSTM step was fed.  Issued behind the encoder tail, whose launch writes those rows."""
        if self.semantic is None:
            return
        a, E, G, ldG = self.arena, self.E, self.G, self.ldG
        x = self._route.xin_used
        self.gemm_sk(x, a.p("guse_out/kernel"), self.sem_z, B, G, E, E, ldG, ldG, bias=a.p("guse_out/bias"))
        k, sem = SemanticTarget.SLOT, self.semantic
        if sem.contrastive:
            # tnt_contrastive_loss_f32 in the cosine launch's place: its means (loss, top1) are adjacent, the slots of ``met``
            # are not (6 and 5), so one two-word launch files them
            soft = 0.0 if sem.soft_temperature is None else 1.0 / sem.soft_temperature
            self.be.contrastive_loss(self.sem_z, ldG, self.sem_g, ldG, self.sem_z if want_grad else None, self.sem_work,
                                     self.sem_loss, self.sem_hit, self.sem_out, B, G, 1.0 / sem.temperature, soft, sem.symmetric,
                                     sem.weight)
            k1 = SemanticTarget.TOP1_SLOT
            self.be.sum2(self.sem_out[0:1], self.met[k:k + 1], self.sem_out[1:2], self.met[k1:k1 + 1], 1, 1.0)
            return
        self.be.cosine_loss(self.sem_z, ldG, self.sem_g, ldG, self.sem_z if want_grad else None, self.sem_loss, self.sem_cos,
                            self.met[k:k + 1], B, G, sem.weight / B)

    def _semantic_bwd_w(self, B):
        """the layer's gradients: dW = x^T dz with the bias gradient as the column-sum rider where the route offers it"""
        if self.semantic is None:
            return
        a, E, G, ldG = self.arena, self.E, self.G, self.ldG
        x, dz = self._route.xin_used, self.sem_z
        if self.g3_riders and self.gemm3(x, dz, a.g("guse_out/kernel"), E, G, B, E, ldG, ldG, transA=True,
                                         colsum=a.g("guse_out/bias")):
            return
        self.gemm_sk(x, dz, a.g("guse_out/kernel"), E, G, B, E, ldG, ldG, transA=True)
        self.be.colsum(dz, a.g("guse_out/bias"), B, G, ldG, self.work2)

    def _semantic_bwd_x(self, B):
        """dXin[:B] += dz W^T, an accumulating product on the stream that wrote dXin (the pair launch of _bwd_seq_lstm or the
        product at the top of _bwd_seq_front) and in front of the tail backward that reads it"""
        if self.semantic is None:
            return
        a, E, G, ldG = self.arena, self.E, self.G, self.ldG
        self.gemm_sk(self.sem_z, a.p("guse_out/kernel"), self.dXin, B, E, G, ldG, ldG, E, transB=True, accumulate=True)

    def _infer_encode(self, B, x):
        """the inference encoder (dense_img, LeakyReLU, BatchNorm / LayerNorm on the moving statistics) of the rows ``x``
        into Xin[:B]"""
        be, a = self.be, self.arena
        N, E = self.N, self.E
        self.gemm_sk(x, a.p("dense_img/kernel"), self.enc_y, B, E, N, self.ldx, E, E, bias=a.p("dense_img/bias"),
                     pre=self.enc_pre, act=ACT_LEAKY, slope=0.2)
        if self.norm == "batch":
            be.batchnorm_fwd(self.enc_y, a.p("batch_norm/gamma"), a.p("batch_norm/beta"), self.mov_mean, self.mov_var,
                             self.Xin, self.xhat, self.inv_std, B, E, E, False, BN_EPS, BN_MOMENTUM, self.work)
        else:
            be.layernorm_fwd(self.enc_y, a.p("batch_norm/gamma"), a.p("batch_norm/beta"), self.Xin, self.xhat,
                             self.inv_std, B, E, E, BN_EPS)

    def predict_embedding(self, betas):
        """The predicted sentence embedding z = x W + bias of the scans ``betas`` (B, n_voxels) -> (B, dim) float32 on the
        model's device, x the inference encoder's feature row (what a decode feeds its feature step): the encoder and one
        product, no decoder step and no decode buffer.  Not normalised: evaluate.semantic_retrieve divides by the norms."""
        if self.semantic is None:
            raise ValueError("predict_embedding needs a model built with semantic=model_base.SemanticTarget(...)")
        xs = self._to_dev(betas, torch.float32)
        if xs.dim() != 2 or xs.shape[1] != self.N:
            raise ValueError(f"betas shape {tuple(xs.shape)} != (batch, {self.N})")
        B = int(xs.shape[0])
        self._build(B, self._shape[1] if self._shape is not None and self._shape[0] == B else 1)
        self.x[:, :self.N].copy_(xs)
        a, E, G, ldG = self.arena, self.E, self.G, self.ldG

        def run():
            self._infer_encode(B, self.x)
            self.gemm_sk(self.Xin, a.p("guse_out/kernel"), self.sem_z, B, G, E, E, ldG, ldG, bias=a.p("guse_out/bias"))
        self._run_captured(("embed", B), run)
        return self.sem_z[:, :G].clone()

    # ------------------------------------------------------------------ forward
    def _forward(self, B, T, training, ss=False):
        """``ss``: the scheduled-sampling training forward (_forward_ss) behind the Embedding gather"""
        be, a = self.be, self.arena
        N, U, E, V, ldV = self.N, self.U, self.E, self.V, self.ldV
        R1 = (T + 1) * B
        sd, ds = self.seed, self.drop_step
        x = self.x
        if training and self.r_in > 0:                                              # NIC.py:122
            be.dropout(self.x, self.xd, B, N, self.ldx, 0, N, 0, self.r_in, sd, S_IN, 0, ds)
            x = self.xd
        drop_l = training and self.r_lstm > 0
        xin = self.Xin_d if drop_l else self.Xin
        fused = self._fused_tail(B)
        stream = fused and self.enc_part is not None
        emb_ride = False
        if stream:      # :125-128 + the feature step's LSTM input dropout: the streaming product's K-split partials are
            #             summed (+ bias, LeakyReLU) by the tail kernel, which holds whole columns for the batch statistics
            self._enc_gram = None
            staged = bool(training and self._route.stage_fwd_done)      # train_step: the staging launch ran this product
            if training and self._gram_fwd(B):
                # the optimizer step will take this kernel's gradient X^T dpre without writing it: leave X X^T and
                # sum W^2 behind, from which (with dpre) its clip-by-norm factor follows (tnt_dense_gram_norm_f32)
                self._gram_bufs()
                if not staged:
                    be.dense_fwd_stream_gram(x, a.p("dense_img/kernel"), self.enc_part, self.enc_gx, self.enc_w2, B, E, N,
                                             self.ldx, E, ENC_SPLITS)
                self._enc_gram = EncGram(pre=self.enc_pre, bias=a.p("dense_img/bias"), gx=self.enc_gx, nsplit=ENC_SPLITS,
                                         w2=self.enc_w2, nw2=ENC_SPLITS * (E // 32))
            elif staged:
                raise RuntimeError("the staging launch ran the Gram form of the encoder forward, which this step does not take")
            else:
                be.dense_fwd_stream(x, a.p("dense_img/kernel"), self.enc_part, B, E, N, self.ldx, E, ENC_SPLITS)
            emb_ride = E % 4 == 0
            targs = (self.enc_part, ENC_SPLITS, a.p("dense_img/bias"), self.enc_pre, 0.2, a.p("batch_norm/gamma"),
                     a.p("batch_norm/beta"), self.mov_mean, self.mov_var, xin, self.xhat, self.inv_std, B, E, E, training,
                     BN_EPS, BN_MOMENTUM, self.r_feat if training else 0.0, self.r_lstm if training else 0.0, sd, S_FEAT,
                     S_LSTM_IN + 0, ds)
            if emb_ride:    # ... with the Embedding gather (+ the text call's input dropout) of the rows behind the features
                be.enc_tail_fwd_sk_emb(*targs, a.p("emb_text/embeddings"), self.cap, xin[B:], B, T, V,
                                       self.r_lstm if drop_l else 0.0, S_LSTM_IN + 1)
            else:
                be.enc_tail_fwd_sk(*targs)
        else:
            self.gemm_sk(x, a.p("dense_img/kernel"), self.enc_y, B, E, N, self.ldx, E, E, bias=a.p("dense_img/bias"),
                         pre=self.enc_pre, act=ACT_LEAKY, slope=0.2)                          # :125
        y = self.enc_y
        if stream:
            pass
        elif fused:     # :126-128 + the feature step's LSTM input dropout in one launch
            be.enc_tail_fwd(y, a.p("batch_norm/gamma"), a.p("batch_norm/beta"), self.mov_mean, self.mov_var, xin,
                            self.xhat, self.inv_std, B, E, E, training, BN_EPS, BN_MOMENTUM,
                            self.r_feat if training else 0.0, self.r_lstm if training else 0.0, sd, S_FEAT,
                            S_LSTM_IN + 0, ds)
        else:
            if training and self.r_feat > 0:                                            # :126
                be.dropout(self.enc_y, self.enc_yd, B, E, E, 0, E, 0, self.r_feat, sd, S_FEAT, 0, ds)
                y = self.enc_yd
            if self.norm == "batch":                                                    # :127-128
                self._bn_fwd(y, a.p("batch_norm/gamma"), a.p("batch_norm/beta"), self.mov_mean, self.mov_var,
                             self.Xin, self.xhat, self.inv_std, B, E, E, training, self.work)
            else:
                be.layernorm_fwd(y, a.p("batch_norm/gamma"), a.p("batch_norm/beta"), self.Xin, self.xhat,
                                 self.inv_std, B, E, E, BN_EPS)
        if drop_l and not fused:
            be.dropout(self.Xin, self.Xin_d, B, E, E, 0, E, 0, self.r_lstm, sd, S_LSTM_IN + 0, 0, ds)
        if stream and emb_ride:
            pass                        # gathered by the tail launch above
        elif drop_l and E % 4 == 0:     # :131 + the text call's LSTM(dropout=...) input mask in one launch
            be.embedding_fwd_drop(a.p("emb_text/embeddings"), self.cap, None, self.Xin_d[B:], B, T, E, E, V, self.r_lstm,
                                  sd, S_LSTM_IN + 1, 0, ds)
        else:
            be.embedding_fwd(a.p("emb_text/embeddings"), self.cap, self.Xin[B:], B, T, E, E, V)   # :131
            if drop_l:       # LSTM(dropout=...) masks the layer input, one mask per call
                be.dropout(self.Xin[B:], self.Xin_d[B:], T * B, E, E, B, E, 0, self.r_lstm, sd, S_LSTM_IN + 1, 0, ds)
        self._route.xin_used = xin
        if ss:
            self._forward_ss(B, T, xin, drop_l)
            return
        # input projection of all T+1 steps as ONE epilogue-free GEMM; the LSTM bias is added inside the step kernel
        if self.fused_xproj and hasattr(be, "gemm_fused") and be.gemm_fused_cfg(R1, 4 * U, E) > 0:
            be.gemm_fused(xin, a.p("lstm/kernel"), self.XZ, R1, 4 * U, E, E, 4 * U, 4 * U)
        else:
            self.gemm_sk(xin, a.p("lstm/kernel"), self.XZ, R1, 4 * U, E, E, 4 * U, 4 * U)
        Ur, bl = a.p("lstm/recurrent_kernel"), a.p("lstm/bias")
        compact = bool(training and self._route.head_map_fresh)       # _head_map_bufs: Out and logits hold the distinct rows
        # both LSTM calls: the feature, one unmasked step (NIC.py:138), and the text, masked by the Embedding mask (:140)
        lstm_layer_fwd(be, self.XZ, self.Hs, self.Cs, Ur, bl, self.cap, T, 1, self.Out, self.gates, T + 1, B, U,
                       chain=self._seq_chain(), out_pos=self.head_pos if compact else None)
        if compact:
            # rows [0, live) only; the tile is planned for the live count seen at the warm-up step (any count is correct)
            self.gemm3(self.Out, a.p("time_distributed_softmax/kernel"), self.logits, T * B, V, U, U, ldV, ldV,
                       bias=a.p("time_distributed_softmax/bias"), live=self.head_live, live_mode=LIVE_ROWS_M,
                       plan_M=self._head_plan_rows(T * B))
            return
        self.gemm_sk(self.Out, a.p("time_distributed_softmax/kernel"), self.logits, T * B, V, U, U, ldV, ldV,
                bias=a.p("time_distributed_softmax/bias"))                         # NIC.py:143

    def _head_plan_rows(self, n):
        """the row count the head forward's tile is planned for: the live count of the warm-up batch plus 3 % (batches of the
        same data differ a little), or n when none was read"""
        est = self._head_live_est
        if est is None or est <= 0:
            return n
        return min(n, est + max(est // 32, 1))

    def _forward_ss(self, B, T, xin, drop_l):
        """The scheduled-sampling forward behind the teacher-forced Embedding gather: XZ of the feature and start-token
        rows, then per LSTM step t the per-step LSTM kernel (gates, Hs, Cs, Out as the per-step fallback writes them), the
        B-row head GEMM into the step's logits rows, and (t <= T-1) tnt_scheduled_feedback_f32, which decides token
        position t of every row, writes a fed token into cap, its masked Embedding row into xin and its projection into
        XZ for step t+1.  The loss, its targets (tgt) and the whole backward are the teacher-forced ones, over the fed ids."""
        be, a = self.be, self.arena
        ss = self.scheduled_sampling if self.scheduled_sampling is not None else self._rollout_ss
        U, E, V, ldV = self.U, self.E, self.V, self.ldV
        Wl, Ur, bl = a.p("lstm/kernel"), a.p("lstm/recurrent_kernel"), a.p("lstm/bias")
        Wo, bo = a.p("time_distributed_softmax/kernel"), a.p("time_distributed_softmax/bias")
        table = a.p("emb_text/embeddings")
        self.gemm_sk(xin, Wl, self.XZ, 2 * B, 4 * U, E, E, 4 * U, 4 * U)
        step = lambda s: lstm_layer_step_fwd(be, s, self.XZ, self.Hs, self.Cs, Ur, bl, self.cap, T, 1, self.Out, self.gates,
                                             B, U)
        step(0)
        rate = self.r_lstm if drop_l else 0.0
        for t in range(1, T + 1):
            step(t)
            logits = self.logits[(t - 1) * B:t * B]
            self.gemm_sk(self.Out[t - 1], Wo, logits, B, V, U, U, ldV, ldV, bias=bo)
            if t < T:
                be.scheduled_feedback(logits, ldV, V, table, E, Wl, 4 * U, 4 * U, self.cap, T, t, xin[(t + 1) * B:], E,
                                      self.XZ[(t + 1) * B:], 4 * U, B, rate, self.seed, S_LSTM_IN + 1, 0, self.drop_step,
                                      T * E, t * E, ss.kind_id, ss.mode_id, self.ss_sched, self.adam_t,
                                      S_SS_COIN + t - 1, S_SS_DRAW + t - 1)

    def _loss_metrics(self, B, T, want_grad):
        """softmax + per-timestep mean CE / accuracy summed over T and divided by T
        (NIC.py:233-240) == sum over all (b,t) / (B*T)."""
        n = T * B
        if want_grad and self._route.head_map_fresh:
            # the distinct rows, each weighted by its multiplicity; rows past the live count hold zeros (staging launch)
            self.be.softmax_cce_live(self.logits, self.head_tgt, None, self.loss_row, self.corr_row, self.logits, n, self.V,
                                     self.ldV, self._head_gscale(n), self.head_live, self.head_w)
        else:
            self._head_loss(B, T, want_grad)
        self._sum2(self.loss_row, self.met[0:1], self.corr_row, self.met[1:2], n, 1.0 / n)
        if want_grad and self._distill_on():
            self._distill_metric(n)

    # ------------------------------------------------------------------ backward
    def _backward(self, B, T):
        self._bwd_head(B, T, join=False)       # dW of the head keeps running beside the BPTT chain
        self._semantic_bwd_w(B)
        self._bwd_seq(B, T, join=False)
        self._bwd_enc(B, T)
        self.join()

    def _bwd_head(self, B, T, join=True):
        """vocabulary head: dW, db, dX (gradients ready first -> first all-reduce bucket under DP)."""
        be, a = self.be, self.arena
        U, V, ldV = self.U, self.V, self.ldV
        dlog = self.logits
        Wo = a.p("time_distributed_softmax/kernel")
        dw = dict(A=self.Out, B=dlog, C=a.g("time_distributed_softmax/kernel"), M=U, N=V, K=T * B, lda=U, ldb=ldV, ldc=ldV,
                  transA=True, colsum=a.g("time_distributed_softmax/bias"))
        dx = dict(A=dlog, B=Wo, C=self.dOut, M=T * B, N=U, K=V, lda=ldV, ldb=ldV, ldc=U, transB=True)
        route = self._route
        route.colsum_deferred = None
        if self._skip_grad("time_distributed_softmax/kernel", "time_distributed_softmax/bias"):
            # a frozen head: the input gradient alone -- no dW / dx pair, no column sums, now or deferred
            if route.head_map_fresh:        # dlogits holds the `live` rows: the compacted head's own dx launch
                self.gemm3(dlog, Wo, self.dOut, T * B, U, V, ldV, ldV, U, transB=True, live=self.head_live,
                           live_mode=LIVE_ROWS_M)
            elif not (self.g3_riders and self.gemm3(dlog, Wo, self.dOut, T * B, U, V, ldV, ldV, U, transB=True)):
                self.gemm_sk(dlog, Wo, self.dOut, T * B, U, V, ldV, ldV, U, transB=True)
            if join:
                self.join()
            return
        if route.head_map_fresh:
            # dlogits and Out hold `live` rows: dW and db sum over those (each already carries its multiplicity), dOut is
            # formed for those; one device word bounds both products
            dw.update(live=self.head_live, live_mode=LIVE_ROWS_K)
            dx.update(live=self.head_live, live_mode=LIVE_ROWS_M)
            rows = self._head_plan_rows(T * B)       # both products are planned, together, for the rows expected to exist
            if not self.gemm3_pair(dict(dw, plan_M=rows), dict(dx, plan_M=rows)):
                self.gemm3(dw["A"], dw["B"], dw["C"], U, V, T * B, U, ldV, ldV, transA=True, colsum=dw["colsum"],
                           live=self.head_live, live_mode=LIVE_ROWS_K)
                self.gemm3(dlog, Wo, self.dOut, T * B, U, V, ldV, ldV, U, transB=True, live=self.head_live,
                           live_mode=LIVE_ROWS_M)
            if join:
                self.join()
            return
        if self.g3_riders and self.gemm3_pair(dw, dx):
            # kernel gradient (with the bias gradient as a rider on the dlogits tiles it streams anyway) and input gradient,
            # the two independent readers of dlogits, in ONE launch
            if join:
                self.join()
            return
        if self.g3_riders and self.gemm3(self.Out, dlog, a.g("time_distributed_softmax/kernel"), U, V, T * B, U, ldV, ldV,
                                         transA=True, colsum=a.g("time_distributed_softmax/bias")):
            pass        # dW and the bias gradient: one launch
        elif self.fused_head_grads and hasattr(be, "gemm_fused") and \
                be.gemm_fused_cfg(U, V, T * B, True, False, 1) > 0:
            be.gemm_fused(self.Out, dlog, a.g("time_distributed_softmax/kernel"), U, V, T * B, U, ldV, ldV, transA=True,
                          colsum=a.g("time_distributed_softmax/bias"))
        else:
            with self.side(0 if self.side_head else -1):
                self.gemm_sk(self.Out, dlog, a.g("time_distributed_softmax/kernel"), U, V, T * B, U, ldV, ldV, transA=True,
                             ws=1)
                if self._tail.deferring and T * B <= 2048:
                    # single-process step: the head-bias column sums share a launch with the LSTM-bias ones behind the
                    # BPTT chain (dlogits stays in place until the next forward)
                    route.colsum_deferred = (dlog, a.g("time_distributed_softmax/bias"), T * B, V, ldV)
                else:
                    be.colsum(dlog, a.g("time_distributed_softmax/bias"), T * B, V, ldV, self.work2)
        self.gemm_sk(dlog, Wo, self.dOut, T * B, U, V, ldV, ldV, U, transB=True)
        if join:
            self.join()

    def _bwd_seq(self, B, T, join=True):
        """BPTT, LSTM / embedding / BatchNorm gradients, down to dpre of the encoder Dense."""
        self._bwd_seq_lstm(B, T)
        self._bwd_seq_front(B, T)
        if join:
            self.join()

    def _bwd_seq_lstm(self, B, T):
        """BPTT over the T+1 LSTM steps and the three LSTM parameter gradients."""
        be, a = self.be, self.arena
        N, U, E, V, ldV = self.N, self.U, self.E, self.V, self.ldV
        R1 = (T + 1) * B
        sd, ds = self.seed, self.drop_step
        route = self._route
        lstm_layer_bwd(be, a.p("lstm/recurrent_kernel"), self.dOut, self.cap, T, 1, self.gates, self.Cs, self.dZ,
                       (self.da_pass, self.dc, self.dout), T + 1, B, U, chain=self._seq_chain(bwd=True),
                       dout_pos=self.head_pos if route.head_map_fresh else None, pass_out_last=False)
        xin, d = route.xin_used, route.colsum_deferred      # d: the head-bias column sums _bwd_head left to this method
        route.dxin_done = False
        if self._skip_grad("lstm/kernel", "lstm/recurrent_kernel", "lstm/bias"):
            # a frozen LSTM: none of its three parameter gradients; _bwd_seq_front forms dXin alone
            if d is not None:
                be.colsum(*d, self.work2)
            return
        riders = self.g3_riders and E == U
        one = False         # kernel, recurrent-kernel and bias gradients went out as ONE launch
        if riders:
            dw = dict(A=xin, B=self.dZ, C=a.g("lstm/kernel"), M=E, N=4 * U, K=R1, lda=E, ldb=4 * U, ldc=4 * U, transA=True,
                      colsum=a.g("lstm/bias"), A2=self.Hs, C2=a.g("lstm/recurrent_kernel"))
            dx = dict(A=self.dZ, B=a.p("lstm/kernel"), C=self.dXin, M=R1, N=E, K=4 * U, lda=4 * U, ldb=4 * U, ldc=E, transB=True)
            # the LSTM's three parameter gradients AND its input gradient (the four readers of dZ) in ONE launch;
            # _bwd_seq_front finds dXin done
            one = route.dxin_done = bool(self.gemm3_pair(dw, dx))
        if riders and not one:
            # the two products share dZ, the column sums of dZ ride on the fragments the first tile row holds anyway
            one = bool(self.gemm3(xin, self.dZ, a.g("lstm/kernel"), E, 4 * U, R1, E, 4 * U, 4 * U, transA=True,
                                  colsum=a.g("lstm/bias"), A2=self.Hs, C2=a.g("lstm/recurrent_kernel")))
        if not one and self.fused_lstm_grads and E == U and hasattr(be, "gemm_fused") and \
                be.gemm_fused_cfg(U, 4 * U, R1, True, False, 2) > 0:
            # ... or in ONE launch of the one-round GEMM family: the bias gradient (column sums of dZ) rides on the tiles the
            # first row of workgroups loads anyway
            be.gemm_fused(xin, self.dZ, a.g("lstm/kernel"), E, 4 * U, R1, E, 4 * U, 4 * U, transA=True,
                          colsum=a.g("lstm/bias"), A2=self.Hs, C2=a.g("lstm/recurrent_kernel"))
            one = True
        if one:
            if d is not None:
                be.colsum(*d, self.work2)
            return
        with self.side(1):
            self.gemm_sk(self.Hs, self.dZ, a.g("lstm/recurrent_kernel"), U, 4 * U, R1, U, 4 * U, 4 * U, transA=True, ws=2)
        with self.side(0):
            self.gemm_sk(xin, self.dZ, a.g("lstm/kernel"), E, 4 * U, R1, E, 4 * U, 4 * U, transA=True, ws=1)
            if d is not None and R1 <= 2048:
                be.colsum2(*d, self.dZ, a.g("lstm/bias"), R1, 4 * U, 4 * U)
            else:
                if d is not None:
                    be.colsum(*d, self.work2)
                be.colsum(self.dZ, a.g("lstm/bias"), R1, 4 * U, 4 * U, self.work2)

    def _bwd_seq_front(self, B, T):
        """LSTM input gradient -> embedding rows, BatchNorm, encoder activation, encoder bias."""
        be, a = self.be, self.arena
        N, U, E, V, ldV = self.N, self.U, self.E, self.V, self.ldV
        R1 = (T + 1) * B
        sd, ds = self.seed, self.drop_step
        if not self._route.dxin_done:
            self.gemm_sk(self.dZ, a.p("lstm/kernel"), self.dXin, R1, E, 4 * U, 4 * U, 4 * U, E, transB=True)
        self._semantic_bwd_x(B)
        fused = self._fused_tail(B)
        if self.r_lstm > 0:
            if not fused:
                be.dropout(self.dXin, self.dXin, B, E, E, 0, E, 0, self.r_lstm, sd, S_LSTM_IN + 0, 0, ds)
        # The text call's LSTM-input dropout' shares a launch with the encoder tail backward (both read the dXin the GEMM above
        # just wrote, different rows), which then runs in front of the Embedding backward.  (Riding on the sparse Embedding
        # backward instead was measured slower, 0.5761 -> 0.5845 ms/step: the Philox calls landed on the few workgroups that
        # own heavily duplicated ids, on the step's critical path.)
        ride = self.r_lstm > 0 and fused and E % 4 == 0
        if ride:
            be.enc_tail_bwd_drop(self.dXin, self.xhat, a.p("batch_norm/gamma"), self.inv_std, self.enc_pre, self.dpre,
                                 a.g("batch_norm/gamma"), a.g("batch_norm/beta"), a.g("dense_img/bias"), B, E, E,
                                 self.r_feat, self.r_lstm, 0.2, sd, S_FEAT, S_LSTM_IN + 0, ds,
                                 self.dXin[B:], T * B, E, E, B, E, 0, self.r_lstm, S_LSTM_IN + 1)
        elif self.r_lstm > 0:
            be.dropout(self.dXin[B:], self.dXin[B:], T * B, E, E, B, E, 0, self.r_lstm, sd, S_LSTM_IN + 1, 0, ds)
        self._route.emb_rows = (self.dXin[B:], T * B, E, E, "emb_text/embeddings")
        # id 0 is the Embedding's mask (mask_zero, NIC.py:77) and the text LSTM honours it: a masked step hands no gradient to
        # its input row, so the rows of id 0 are zero (BPTT leaves dz = 0 there and dXin = dz W^T)
        self._embedding_bwd(self.dXin[B:], self.cap, "emb_text/embeddings", B, T, E, E, V, zero_id=0)
        if ride:
            return
        if fused:       # dropout' -> BatchNorm' -> dropout' -> LeakyReLU' -> dpre, encoder bias gradient: one launch
            be.enc_tail_bwd(self.dXin, self.xhat, a.p("batch_norm/gamma"), self.inv_std, self.enc_pre, self.dpre,
                            a.g("batch_norm/gamma"), a.g("batch_norm/beta"), a.g("dense_img/bias"), B, E, E,
                            self.r_feat, self.r_lstm, 0.2, sd, S_FEAT, S_LSTM_IN + 0, ds)
            return
        if self.norm == "batch":
            self._bn_bwd(self.dXin, self.xhat, a.p("batch_norm/gamma"), self.inv_std, self.dyd,
                         a.g("batch_norm/gamma"), a.g("batch_norm/beta"), B, E, E, self.work)
        else:
            be.layernorm_bwd(self.dXin, self.xhat, a.p("batch_norm/gamma"), self.inv_std, self.dyd,
                             a.g("batch_norm/gamma"), a.g("batch_norm/beta"), B, E, E, self.work)
        if self.r_feat > 0:
            be.dropout(self.dyd, self.dyd, B, E, E, 0, E, 0, self.r_feat, sd, S_FEAT, 0, ds)
        be.act_bwd(self.enc_pre, self.dyd, self.dpre, B * E, ACT_LEAKY, 0.2)
        be.colsum(self.dpre, a.g("dense_img/bias"), B, E, E, self.work)

    def _bwd_enc(self, B, T, x_all=None, dpre_all=None):
        """encoder kernel gradient dW = X^T dpre.  Under DP the operands of all ranks are passed
        (all-gathered: 5 MB of betas + 128 KB per rank) and every rank computes the full global-batch
        gradient itself, instead of all-reducing the 41 MB result."""
        be, a = self.be, self.arena
        if x_all is None and self._skip_grad("dense_img/kernel"):     # a frozen encoder kernel: no product, no fused update, no Gram norm
            self._enc_last_fused = None
            return
        x = self.xd if self.r_in > 0 else self.x
        rows = B
        if x_all is not None:
            x, dpre, rows = x_all, dpre_all, x_all.shape[0]
        else:
            dpre = self.dpre
        self._enc_last_fused = None
        if x_all is None and self._enc_update_fused(rows):
            self._tail.enc = EncUpdate("dense_img/kernel", x, dpre, rows, self.N, self.E, self.ldx,
                                       gram=self._enc_gram)                       # -> _update_fused
            self._enc_last_fused = (x, dpre, rows)       # train_step marks the gradient buffer stale after every (re)play
            return
        if rows <= 64 and self.E % 16 == 0:
            be.dense_dw_skinny(x, dpre, a.g("dense_img/kernel"), self.N, self.E, rows, self.ldx)
        else:
            self.gemm_sk(x, dpre, a.g("dense_img/kernel"), self.N, self.E, rows, self.ldx, self.E, self.E, transA=True)

    # ---- row-sharded update of the encoder kernel under data parallel (dp.PipelinedDenseSync(shard_encoder=True)): rank r forms
    # rows [r0, r0 + nr) of dW = X_all^T dpre_all from the gathered operands (N / G rows: the single-process product's work
    # instead of G times it), the variable's clip norm is one 8-byte all-reduce of the shards' (sum g^2, sum theta^2), Adam runs
    # on the shard (1 / G of the 246 MB the update of this variable moves) and the updated rows are all-gathered.
    def _enc_shard_state(self, r0, nr):
        st = self._enc_shard
        if st is None or st["key"] != (r0, nr):
            from .arena import build_spans
            a, e = self.arena, self.arena.entries["dense_img/kernel"]
            assert e.seg == 0 and e.off == 0
            sp = build_spans([e.off + r0 * self.E], [nr * self.E], self.device)
            st = self._enc_shard = dict(key=(r0, nr), sp=sp, scratch=self._f(2 * sp.nspan), send=self._f(nr * self.E))
            a.partial[:2 * a.spans.first_host[1]].zero_()          # the variable's slots: only [0:2] carries data from here on
        return st

    def _enc_shard_grad(self, x_all, dpre_all, r0, nr):
        """rows [r0, r0 + nr) of the encoder kernel's global-batch gradient + the shard's norm pair -> arena.partial[0:2]"""
        be, a = self.be, self.arena
        st = self._enc_shard_state(r0, nr)
        sp = st["sp"]
        rows = x_all.shape[0]
        self.gemm_sk(x_all[:, r0:], dpre_all, a.g("dense_img/kernel")[r0:r0 + nr], nr, self.E, rows, self.ldx, self.E, self.E,
                     transA=True)
        be.seg_sqnorm(a.theta, a.grad, sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, a.seg_l2, st["scratch"],
                      a.partial[0:1], a.partial[1:2], None, sp.nspan, 1)

    def _enc_shard_adam(self, r0, nr):
        """clip (norm of the WHOLE variable: arena.partial[0], all-reduced) + Adam on the shard; the updated rows -> send buffer"""
        be, a, opt = self.be, self.arena, self.optimizer
        st = self._enc_shard_state(r0, nr)
        sp = st["sp"]
        clip = opt.clipnorm if opt.clipnorm is not None else 0.0
        be.adam(a.theta, self.opt_m, self.opt_v, a.grad, sp.span_seg, sp.span_off, sp.span_len, a.seg_l2, a.partial[0:1],
                a.sq_override, sp.nspan, 0.0, self.lr_t_dev, opt.beta_1, opt.beta_2, opt.epsilon, clip, guard=self._guard_word())
        return st["send"]

    # ------------------------------------------------------------------ steps
    def _train_graph(self, B, T):
        self._forward(B, T, True, ss=self.scheduled_sampling is not None)
        self._loss_metrics(B, T, True)
        self._semantic_fwd(B, True)
        self._backward(B, T)

    def train_step(self, data):
        """NIC.train_step (NIC.py:198-252): data = ((betas, cap, a0, c0), target).  With ``self_critical`` set, the
        self-critical step (train_step_scst) instead."""
        if self.optimizer is None:
            raise RuntimeError("compile() the model before train_step")
        compat.check(self, self.STEP_FEATURES)       # (grad_sync may have been attached since the constructor)
        if self.self_critical is not None:
            return self.train_step_scst(data)
        self._sync_accum()
        distill = self._distill_begin()
        # a micro-step of an accumulation window stages as the generic data-parallel step does: the forward does not ride in
        # the staging launch and the head keeps its position-ordered rows; so does a distilled step (the staging launch's
        # encoder forward needs the row map beside it)
        plain = self.grad_sync is None and self._accum_k() is None and not distill
        guse = self._semantic_target(data[0])
        B, T = self._stage_batch(data[0], data[1], self.N, head_map=plain, fwd=plain, corrupt=True)
        self._semantic_stage(guse)
        self._ss_refuse(T)
        if distill:
            self._teach(data, B, T)
            self._distill_bufs(B, T)        # behind it: the teacher may just have rebuilt its buffers
        self._sync_lr()
        self._enc_grad_stale = None
        ring = False
        if self._accum_host is not None:    # gradient_accumulation_steps=k: ModelBase._train_step_accum
            if self._train_step_accum(B, T):
                self.optimizer.iterations += 1
            return self._lr_metric(self._metrics_from(self._met_snapshot(), loss=0, L2=2, accuracy=1))
        if self.grad_sync is None:      # replayed as a launch plan or a hipGraph: ModelBase._step_runner
            compact = self._route.head_map_fresh        # the staging launch built the head's row map
            staged = self._route.stage_fwd_done         # ... and ran the encoder forward: the step leaves it out
            key = ("train", B, T, "compact") if compact else ("train", B, T, "distill") if distill else ("train", B, T)
            if self.semantic is not None:       # the step with the term is another launch sequence, and so is each loss
                key += self._semantic_key()
            seen = self._plan_staged
            if self._graphs.get(key) is not None and seen.get(key) != staged:
                del self._graphs[key]       # recorded with / without the forward (the entry refuses by alignment): start over
            seen[key] = staged
            if compact and self._head_live_est is None and self._graphs.get(key) is None:
                # the eager warm-up step synchronises anyway: read the live count once, for the head forward's tile only
                self._head_live_est = int(self.head_live.item())
            ring = self._run_step(self._step_runner(), key, lambda: self._train_and_update_graph(B, T))
            self._enc_grad_stale = self._enc_last_fused
        elif getattr(self.grad_sync, "pipelined", False):
            self.grad_sync.step(self, B, T)
        else:
            self._train_step_dp(B, T, lambda: self._train_graph(B, T), self._update_graph)
        self.optimizer.iterations += 1
        m = self._met_snapshot(ring)
        kl = dict(distill_kl=self.DISTILL_KL) if distill else {}
        kl.update(self._semantic_slots())
        return self._lr_metric(self._metrics_from(m, loss=0, L2=2, accuracy=1, **kl))

    # ------------------------------------------------------------------ self-critical sequence training
    def _scst_bufs(self, B, T):
        """per (B, T): the B staged rows (betas, state, caption, start token), the greedy ids (T, B), the last sampled
        token and the advantage (R), and the host side of the step's one round trip"""
        R = B * self.self_critical.n_samples
        st = self._scst
        if st is not None and st["key"] == (B, T):
            return st
        f, dev, i32 = self._f, self.device, torch.int32
        pin = self.device.type == "cuda"
        h = lambda *shape, dtype=i32: torch.zeros(*shape, dtype=dtype, pin_memory=pin)
        st = self._scst = dict(key=(B, T), x=f(B, self.ldx), h0=f(B, self.U), c0=f(B, self.U),
                               cap=torch.zeros(B, T, dtype=i32, device=dev), start=torch.zeros(B, 1, dtype=i32, device=dev),
                               greedy=torch.zeros(T, B, dtype=i32, device=dev), last=torch.zeros(R, dtype=i32, device=dev),
                               adv=f(R), h_cap=h(R, T), h_last=h(R), h_greedy=h(T, B), h_ref=h(B, T),
                               h_adv=h(R, dtype=torch.float32))
        if self.self_critical.score_on == "device":
            # tnt_caption_reward_f32's side: the references at the kernel's largest extents, so that the launch is the same
            # whatever a step's references are, the float64 scores and the counted positions
            M, Lr = REWARD_MAX_REFS, REWARD_MAX_LEN
            st.update(refs=torch.zeros(B, M, Lr, dtype=i32, device=dev), n_refs=torch.zeros(B, dtype=i32, device=dev),
                      h_refs=h(B, M, Lr), h_nrefs=h(B), refs_own=False, refs_sent=None,
                      score=torch.zeros(B, self.self_critical.n_samples + 1, dtype=torch.float64, device=dev),
                      counted=torch.zeros(R, dtype=i32, device=dev))
        return st

    def _stage_scst(self, inputs):
        """Stages the B rows of a self-critical step, and their K copies as the R = B*K rows of the step's buffers (row
        b*K + k: copy k of scan b), on the device (a torch copy, at staging: a recorded launch plan re-issues backend
        launches only).  Over K identical copies BatchNorm's batch statistics are those of the B rows; every copy draws its
        own Dropout masks (so with input Dropout the copies, and the statistics, differ)."""
        self._route = StepRoute()
        x, cap, a0, c0 = inputs[:4]
        cap_t = self._to_dev(cap, torch.int32)
        B, T = cap_t.shape
        if T - 1 > SS_MAX_POSITIONS:
            raise ValueError(f"self-critical rollouts sample at most {SS_MAX_POSITIONS} token positions per caption through "
                             f"the scheduled-sampling sites (S_SS_DRAW + j): caption length {T} is too long")
        K = self.self_critical.n_samples
        self._build(B * K, T)
        st = self._scst_bufs(B, T)
        xs = self._to_dev(x, torch.float32)
        assert xs.shape == (B, self.N), f"betas shape {tuple(xs.shape)} != {(B, self.N)}"
        st["x"][:, :self.N].copy_(xs)
        st["h0"].copy_(self._to_dev(a0, torch.float32))
        st["c0"].copy_(self._to_dev(c0, torch.float32))
        st["cap"].copy_(cap_t)
        st["start"].copy_(cap_t[:, :1])
        self.x.view(B, K, self.ldx).copy_(st["x"][:, None, :].expand(B, K, self.ldx))
        self.Hs[0].view(B, K, self.U).copy_(st["h0"][:, None, :].expand(B, K, self.U))
        self.Cs[0].view(B, K, self.U).copy_(st["c0"][:, None, :].expand(B, K, self.U))
        self.cap.view(B, K, T).copy_(cap_t[:, None, :].expand(B, K, T))
        return B, T

    def _scst_greedy(self, B, T):
        """the baseline: greedy_predict's inference-mode decode of the B staged rows for T positions, the argmax ids of
        position i into greedy[i], on slices of the step's buffers (rows [0, B) of enc_y, Xin, XZ, Hs[1..2], Cs[1..2],
        gates[0], Out[0], logits) before the rollout overwrites them"""
        be, a, st = self.be, self.arena, self._scst
        U, V, ldV = self.U, self.V, self.ldV
        h, c = [self.Hs[1][:B], self.Hs[2][:B]], [self.Cs[1][:B], self.Cs[2][:B]]
        self._decode_encode(B, (st["x"], st["h0"], st["c0"], h[0], c[0]))
        xz, emb, out, probs, ids = self.XZ[:B], self.Xin[B:2 * B], self.Out[0][:B], self.logits[:B], st["greedy"]
        for i in range(T):
            tok = st["start"] if i == 0 else ids[i - 1].view(B, 1)
            self._text_step(tok, i == 0, B, emb, xz, h[i & 1], c[i & 1], h[(i & 1) ^ 1], c[(i & 1) ^ 1], out,
                            self.gates[0][:B])
            self.gemm_sk(out, a.p("time_distributed_softmax/kernel"), probs, B, V, U, U, ldV, ldV,
                         bias=a.p("time_distributed_softmax/bias"))
            be.softmax_cce(probs, None, probs, None, None, None, B, V, ldV, 0.0)
            be.argmax_rows(probs, ids[i], B, V, ldV)

    def _scst_rollout(self, R, T):
        """the training forward over the R rows with every token position sampled (_forward_ss at p = 1, sample mode:
        w_1..w_{T-1} into cap[:, 1:]), and the draw of w_T from step T's logits (Philox site S_SCST_LAST)"""
        self._forward(R, T, True, ss=True)
        self.be.sample_rows(self.logits[(T - 1) * R:], self._scst["last"], R, self.V, self.ldV, 1.0, True, self.seed,
                            S_SCST_LAST, 0, self.drop_step)

    def _scst_update(self, R, T):
        """tnt_scst_cce_f32 (loss rows, dlogits in place of the logits), the teacher-forced backward over the sampled ids,
        and the fused update: the L2 terms, the clip and Adam of train_step"""
        st = self._scst
        if self.self_critical.score_on == "device":
            self._scst_reward(R, T)
        with self._deferring():
            self.be.scst_cce(self.logits, self.ldV, self.V, self.cap, T, st["last"], st["adv"], self.self_critical.end_id,
                             self.loss_row, None, self.logits, R, 1.0 / R)
            self._sum2(self.loss_row, self.met[0:1], self.loss_row, self.met[1:2], T * R, 1.0 / R)
            self._backward(R, T)
        self._update_fused(self.met[2:3])

    def _scst_reward(self, R, T):
        """score_on="device": the rewards of the R sampled captions (and the greedy captions) against the staged references
        and the advantages into st["adv"], one tnt_caption_reward_f32 launch on buffers that are static per (B, T); reward
        "rouge-l": one tnt_caption_rouge_f32 launch in its place, on the same buffers"""
        sc, st = self.self_critical, self._scst
        B = R // sc.n_samples
        if sc.reward == ROUGE_KIND:
            g = sc.baseline == "greedy"
            self.be.caption_rouge(self.cap, T, st["last"], st["greedy"] if g else None, B, st["refs"], st["n_refs"],
                                  REWARD_MAX_REFS, REWARD_MAX_LEN, B, sc.n_samples, sc.end_id, ROUGE_BETA, 0 if g else 1,
                                  st["adv"], st["score"], st["counted"])
            return
        keys = idf = params = None
        n_keys = 0
        if sc.table is not None:
            keys, idf, params = sc.table.device(self.device)
            n_keys = len(sc.table)
            if n_keys == 0:
                keys = idf = None
        greedy = sc.baseline == "greedy"
        self.be.caption_reward(self.cap, T, st["last"], st["greedy"] if greedy else None, B, st["refs"], st["n_refs"],
                               REWARD_MAX_REFS, REWARD_MAX_LEN, keys, idf, n_keys, params, B, sc.n_samples, sc.end_id,
                               REWARD_KINDS[sc.reward], 0 if greedy else 1, st["adv"], st["score"], st["counted"])

    def _scst_stage_refs(self, references, B, T):
        """score_on="device": the step's references into st["refs"] (B, 8, 64) / st["n_refs"].  ``references`` None: each
        row's own staged caption, columns 1.., copied on the device (the kernel cuts it at its first end_id or 0);
        else B lists of references, packed into pinned host arrays and copied over without waiting.  More than 8
        references or one longer than 64 tokens raises ValueError, before any launch."""
        st = self._scst
        if references is None:
            if not st["refs_own"]:
                st["refs"].zero_()
                st["n_refs"].fill_(1)
                st["refs_own"] = True
            st["refs"][:, 0, :T - 1].copy_(st["cap"][:, 1:])
            return
        if st["refs_sent"] is not None:
            st["refs_sent"].synchronize()          # the last step's copy has read the pinned arrays (long done)
        pack_references(references, st["h_refs"].numpy(), st["h_nrefs"].numpy())
        st["refs_own"] = False
        st["refs"].copy_(st["h_refs"], non_blocking=True)
        st["n_refs"].copy_(st["h_nrefs"], non_blocking=True)
        if self.device.type == "cuda":
            st["refs_sent"] = torch.cuda.Event()
            st["refs_sent"].record()

    def _scst_round_trip(self, B, T):
        """the step's one synchronisation: sampled (R, T), greedy (T, B) and staged caption (B, T) ids to the host"""
        st = self._scst
        pairs = [(st["h_cap"], self.cap), (st["h_last"], st["last"]), (st["h_ref"], st["cap"])]
        if self.self_critical.baseline == "greedy":
            pairs.append((st["h_greedy"], st["greedy"]))
        for hst, dv in pairs:
            hst.copy_(dv, non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream().synchronize()
        samples = np.concatenate([st["h_cap"].numpy()[:, 1:], st["h_last"].numpy()[:, None]], 1)
        return samples, st["h_greedy"].numpy().T, st["h_ref"].numpy()

    def train_step_scst(self, data, references=None):
        """Self-critical sequence training (Rennie et al. 2017), one step; model_base.SelfCritical holds the definition.
        data = ((betas, cap, a0, c0)[, target]); the target is not used.  ``references``: B lists of tokenised reference
        captions (several per scan); None takes each row's own caption, cap[b, 1:] cut at its first end_id or 0.
        With R = B*K: the B rows are staged and expanded to R on the device (_stage_scst); [greedy baseline: an inference
        decode of the B rows, ids kept on the device]; the rollout: the training forward over the R rows with every token
        sampled (Philox sites S_SS_DRAW + j and S_SCST_LAST, stream step drop_step); one device-to-host copy of the ids,
        the rewards and advantages on the host, the advantages back to the device; then tnt_scst_cce_f32, the backward
        and the update as one recorded segment.  With SelfCritical(score_on="device") the middle stays on the device
        instead: the references are staged beside the batch (_scst_stage_refs) and the update segment opens with one
        tnt_caption_reward_f32 launch that writes the advantages (_scst_device_tail); nothing waits for the stream.
        Each device segment is replayed as a launch plan or a hipGraph like train_step.  Metrics: loss (the policy-gradient loss), L2, reward (mean sampled reward), baseline (mean baseline
        reward), sample_len (mean number of tokens the loss counts)."""
        sc = self.self_critical
        if sc is None:
            raise ValueError("train_step_scst needs a model built with self_critical=model_base.SelfCritical(...)")
        if self.optimizer is None:
            raise RuntimeError("compile() the model before train_step")
        compat.check(self, ("self_critical",))
        B, T = self._stage_scst(data[0])
        if references is not None and len(references) != B:
            raise ValueError(f"references: {len(references)} reference lists for a batch of {B}")
        R = B * sc.n_samples
        if sc.score_on == "device":
            self._scst_stage_refs(references, B, T)
        self._sync_lr()
        self._enc_grad_stale = None
        run = self._step_runner()
        if sc.baseline == "greedy":
            run(("scst_greedy", B, T), lambda: self._scst_greedy(B, T))
        run(("scst_rollout", R, T), lambda: self._scst_rollout(R, T))
        if sc.score_on == "device":
            return self._scst_device_tail(run, B, R, T)
        samples, greedy, cap0 = self._scst_round_trip(B, T)
        if references is None:
            references = [[sc.truncate(row[1:])] for row in cap0]
        adv, reward, base, counted = sc.advantages(samples, references, greedy if sc.baseline == "greedy" else None)
        st = self._scst
        st["h_adv"].copy_(torch.from_numpy(adv.astype(np.float32)))
        st["adv"].copy_(st["h_adv"], non_blocking=True)
        ring = self._run_step(run, ("scst_update", R, T), lambda: self._scst_update(R, T))
        self._enc_grad_stale = self._enc_last_fused
        self.optimizer.iterations += 1
        m = self._met_snapshot(ring)
        return self._lr_metric(self._metrics_from(m, loss=0, L2=2, reward=float(reward.mean()), baseline=float(base.mean()),
                                                  sample_len=float(counted.mean())))

    def _scst_device_tail(self, run, B, R, T):
        """score_on="device": behind the rollout the update segment, whose first launch is tnt_caption_reward_f32 (recorded
        into the segment's plan or hipGraph with it): no id and no reward visits the host and nothing waits for the
        stream.  The reward, baseline and sample_len metrics are means of the kernel's float64 scores and counted
        positions, taken on the device behind the update and read with the step's metrics."""
        sc, st = self.self_critical, self._scst
        K = sc.n_samples
        ring = self._run_step(run, ("scst_update", R, T), lambda: self._scst_update(R, T))
        self._enc_grad_stale = self._enc_last_fused
        self.optimizer.iterations += 1
        m = self._met_snapshot(ring)
        reward = st["score"][:, :K]
        if sc.baseline == "greedy":
            base = st["score"][:, K].mean()
        else:
            base = ((reward.sum(1, keepdim=True) - reward) / (K - 1)).mean()
        return self._lr_metric(self._metrics_from(m, loss=0, L2=2, reward=reward.mean(), baseline=base,
                                                  sample_len=st["counted"].to(torch.float64).mean()))

    def test_step(self, data):
        """NIC.test_step (NIC.py:254-299)."""
        compat.check(self, ("semantic",))
        guse = self._semantic_target(data[0])
        B, T = self._stage_batch(data[0], data[1], self.N)
        self._semantic_stage(guse)
        sem = self.semantic is not None

        def run():
            self._forward(B, T, False)
            self._loss_metrics(B, T, False)
            self._semantic_fwd(B, False)
            self._norms_and_l2(self.met[2:3])
        self._run_captured(("test", B, T) + (self._semantic_key() if sem else ()), run)
        m = self._met_snapshot()
        return self._metrics_from(m, loss=0, L2=2, accuracy=1, **self._semantic_slots())

    def __call__(self, data, training=False):
        """NIC.call (NIC.py:100-145): returns probabilities (B, T, V)."""
        B, T = self._stage_inputs(data)

        def run():
            self._forward(B, T, training)
            return self._probs(B, T)
        return self._guarded(run)

    call = __call__

    def greedy_predict(self, img_input, a0, c0, start_seq, max_len, units=None, tokenizer=None, constraints=None,
                       consensus=None, guidance=None):
        """NIC.greedy_predict (NIC.py:148-195), inference mode; returns np.ndarray (max_len, B, 1, V).
        A predicted id 0 masks the following LSTM step exactly as the keras Embedding mask does.
        ``constraints``, ``consensus``, ``guidance``: model_base.DecodeConstraints, Consensus and Guidance, whose docstrings
        define them.  The returned probabilities are then the constrained distributions; the mixtures, (max_len, M, 1, V)
        for the G * M member-major rows of img_input, a0, c0; the guided distributions.  With consensus or guidance a fed
        0 masks the next LSTM step on every member."""
        probs_all, _ = self._decode(img_input, a0, c0, start_seq, max_len, None, constraints, consensus, guidance)
        return probs_all[:, :, :self.V].cpu().numpy()[:, :, None, :]

    def sample_predict(self, img_input, a0, c0, start_seq, max_len, units=None, tokenizer=None, temperature=1.0,
                       top_k=0, top_p=1.0, sample_step=0, constraints=None, consensus=None, guidance=None):
        """greedy_predict with the argmax replaced by a categorical draw from each step's probabilities, filtered by
        ``top_k`` (>= 1: only the k most likely tokens; 0: off) and ``top_p`` (< 1: only the shortest most-likely prefix
        whose mass reaches top_p; 1: off) at ``temperature`` (tnt_sample_topkp_f32, definition in include/tnt_hip.h).
        The draw is the Philox stream (seed, S_SAMPLE + position, sample_step), as in lc_nic.NIC.sample_predict.  A
        sampled id 0 masks the following LSTM step exactly as a greedy 0 does.  The decode is captured and replayed like
        greedy_predict; sample_step reaches the replay through a device word.
        ``constraints``, ``consensus``, ``guidance`` as in greedy_predict: the draw is from the constrained, mixed or guided
        distribution, which is also what ``probs`` holds then; with consensus ids and probs are per image (M rows).
        Returns (ids (B, max_len, 1) int64, probs (max_len, B, 1, V))."""
        top_k, top_p, temperature = check_sampling(top_k, top_p, temperature)
        probs_all, ids = self._decode(img_input, a0, c0, start_seq, max_len, (temperature, top_k, top_p, int(sample_step)),
                                      constraints, consensus, guidance)
        V = self.V
        ids = ids[:, :probs_all.shape[1]]              # consensus / guidance: member 0's rows (every member holds the common word)
        return (ids.t().contiguous().cpu().numpy().astype(np.int64)[:, :, None],
                probs_all[:, :, :V].cpu().numpy()[:, :, None, :])

    def _decode_encode(self, B, src=None):
        """the inference encoder (dense_img, BatchNorm / LayerNorm) and the feature LSTM step of a decode over the staged
        B rows: the state after the feature step is Hs[1], Cs[1].  ``src`` = (x, h0, c0, h1, c1): other input rows and
        initial state, and where the state after the feature step goes"""
        x, h0, c0, h1, c1 = src if src is not None else (self.x, self.Hs[0], self.Cs[0], self.Hs[1], self.Cs[1])
        self._infer_encode(B, x)
        self._feature_step(self.Xin, B, self.XZ[:B], h0, c0, h1, c1, self.gates[0])

    def _feature_step(self, feat, rows, xz, h_in, c_in, h_out, c_out, gates):
        """the feature step of a decode: the input projection of the encoded rows ``feat`` with the LSTM bias, and one
        unmasked LSTM step h_in, c_in -> h_out, c_out"""
        a, U, E = self.arena, self.U, self.E
        self.gemm_sk(feat, a.p("lstm/kernel"), xz, rows, 4 * U, E, E, 4 * U, 4 * U, bias=a.p("lstm/bias"))
        self.be.lstm_step_fwd(xz, h_in, c_in, a.p("lstm/recurrent_kernel"), None, None, 0, None, 0, 0, None, h_out, c_out,
                              None, gates, rows, U)

    def _text_step(self, words, first, rows, emb, xz, h_in, c_in, h_out, c_out, out, gates):
        """the token step of a decode, three launches: the Embedding gather of the fed ``words`` into ``emb``, its input
        projection with the LSTM bias, and one LSTM step h_in, c_in -> h_out, c_out, `out`, masked by a fed 0 as by the
        keras Embedding mask (a masked row carries its state) unless ``first``: the start token always advances"""
        a, U, E = self.arena, self.U, self.E
        self.be.embedding_fwd(a.p("emb_text/embeddings"), words, emb, rows, 1, E, E, self.V)
        self.gemm_sk(emb, a.p("lstm/kernel"), xz, rows, 4 * U, E, E, 4 * U, 4 * U, bias=a.p("lstm/bias"))
        self.be.lstm_step_fwd(xz, h_in, c_in, a.p("lstm/recurrent_kernel"), None, None, 0, None if first else words, 1, 0,
                              None, h_out, c_out, out, gates, rows, U)

    def _decode(self, img_input, a0, c0, start_seq, max_len, filt, constraints=None, consensus=None, guidance=None):
        """the decode loop of greedy_predict (filt None: argmax) and sample_predict (filt = (temperature, top_k, top_p,
        sample_step)); returns the device buffers (probs (max_len, M, ldV), ids (max_len, B) int32) of the step's choice
        (model_base._TokenChoice).  With consensus or guidance on (ModelBase._decode_setup) the decoder runs the B = G * M
        member rows, probs holds the M mixtures per step and ids the common word on every member row."""
        be, a = self.be, self.arena
        cons, (img_input, a0, c0), start, _, _, B, con, _, ckey = self._decode_setup(
            guidance, consensus, constraints, None, img_input, a0, c0, start_seq, max_len)
        cap = torch.zeros(B, 1, dtype=torch.int32, device=self.device)
        self._stage_inputs((img_input, cap, a0, c0))
        U, V, ldV = self.U, self.V, self.ldV
        # static decode buffers per (B, max_len): the whole loop is one captured hipGraph
        choice = _TokenChoice(self, B, max_len, filt, con, cons)
        choice.start.copy_(start.view(B, 1))

        def run():
            self._decode_encode(B)
            xz, emb = self.XZ[:B], self.Xin[B:2 * B]
            h = [self.Hs[0], self.Hs[1]]
            c = [self.Cs[0], self.Cs[1]]
            cur = 1
            out = self.Out[0]
            words = choice.start
            for i in range(max_len):
                self._text_step(words, i == 0, B, emb, xz, h[cur], c[cur], h[1 - cur], c[1 - cur], out, self.gates[0])
                cur = 1 - cur
                logits = choice.logits(i)
                self.gemm_sk(out, a.p("time_distributed_softmax/kernel"), logits, B, V, U, U, ldV, ldV,
                             bias=a.p("time_distributed_softmax/bias"))
                words = choice.step(i, logits, words)
        if filt is None:
            self._run_captured(("greedy", B, max_len) + ckey, run)
        else:
            self._run_captured(("sample", B, max_len) + tuple(filt[:3]) + ckey, run)
        return choice.probs, choice.ids

    def _mbr_candidate(self, img_input, a0, c0, start_seq, max_len, filt, constraints=None, consensus=None, guidance=None):
        """ModelBase.mbr_decode's candidate decode: sample_predict's or (``filt`` None) greedy_predict's, ids left on the device"""
        return self._decode(img_input, a0, c0, start_seq, max_len, filt, constraints, consensus, guidance)[1]

    # ------------------------------------------------------------------ caption scoring (ModelBase.score_captions)
    def _score_refuse(self):
        if self.grad_sync is not None:
            raise NotImplementedError("score_captions has no data-parallel schedule: score on one device")

    def _score_bufs(self, Rmax, T):
        """decoder buffers of one scoring pass of up to Rmax rows: T-1 LSTM steps, their logits, the kernel's outputs"""
        f, U, E, steps = self._f, self.U, self.E, T - 1
        # the persistent chain (passes of <= 128 rows) keeps the gates of every step, the per-step kernels reuse one slab
        seq_rows = min(Rmax, 128) if self._seq_lstm else 0
        return dict(cap=torch.zeros(Rmax * T, dtype=torch.int32, device=self.device), xin=f(T * Rmax * E),
                    xz=f(steps * Rmax * 4 * U), hs=f((steps + 1) * Rmax * U), cs=f((steps + 1) * Rmax * U),
                    out=f(steps * Rmax * U), gates=f(max(Rmax, steps * seq_rows) * 4 * U), logits=f(steps * Rmax * self.ldV),
                    tok_lp=f(steps * Rmax), cap_lp=f(Rmax), cap_len=torch.zeros(Rmax, dtype=torch.int32, device=self.device))

    def _score_shape(self, st, R, T):
        U, E, steps = self.U, self.E, T - 1
        pre = lambda k, *shape: st[k][:int(np.prod(shape))].view(*shape)
        seq = bool(self._seq_lstm) and R <= 128 and self.be.lstm_seq_supported(R, U)
        return dict(cap=pre("cap", R, T), xin=pre("xin", T * R, E), xz=pre("xz", steps * R, U, 4),
                    hs=pre("hs", steps + 1, R, U), cs=pre("cs", steps + 1, R, U), out=pre("out", steps, R, U),
                    gates=pre("gates", steps, R, U, 4) if seq else pre("gates", R, U, 4),
                    logits=pre("logits", steps * R, self.ldV), tok_lp=pre("tok_lp", steps * R), cap_lp=pre("cap_lp", R),
                    cap_len=pre("cap_len", R), seq=seq)

    def _score_pass(self, B, Cr, T, end_id, v, first):
        """one scoring pass over R = B*Cr decoder rows.  ``first``: the inference encoder and the feature LSTM step of the
        B staged scans (_decode_encode: state in Hs[1], Cs[1]) run in front.  Then: that state gathered to the R rows; the
        Embedding gather and the input projection of the T-1 text steps; the masked LSTM steps (NIC.py:140's Embedding
        mask: a fed 0 carries state and output) as the persistent chain or per step; the head GEMM; and
        tnt_caption_score_f32 on the logits (no softmax launch)."""
        be, a = self.be, self.arena
        U, E, V, ldV = self.U, self.E, self.V, self.ldV
        R, steps = B * Cr, T - 1
        n = steps * R
        if first:
            self._decode_encode(B)
        hs, cs, out, xz, cap = v["hs"], v["cs"], v["out"], v["xz"], v["cap"]
        be.embedding_fwd(self.Hs[1], v["rep"], hs[0], R, 1, U, U, B)
        be.embedding_fwd(self.Cs[1], v["rep"], cs[0], R, 1, U, U, B)
        be.embedding_fwd(a.p("emb_text/embeddings"), cap, v["xin"], R, T, E, E, V)      # t-major; rows [0, n) are used
        self.gemm_sk(v["xin"], a.p("lstm/kernel"), xz, n, 4 * U, E, E, 4 * U, 4 * U)
        Ur, bl = a.p("lstm/recurrent_kernel"), a.p("lstm/bias")
        lstm_layer_fwd(be, xz, hs, cs, Ur, bl, cap, T, 0, out, v["gates"], steps, R, U,
                       chain=self._seq_chain() if v["seq"] else None)
        self.gemm_sk(out, a.p("time_distributed_softmax/kernel"), v["logits"], n, V, U, U, ldV, ldV,
                     bias=a.p("time_distributed_softmax/bias"))
        be.caption_score(v["logits"], ldV, V, cap, T, steps, R, end_id, v["tok_lp"], v["cap_lp"], v["cap_len"])

    def beam_search(self, img_input, a0, c0, start_seq, max_len, beam_width=5, end_id=-1, length_penalty=0.0,
                    units=None, tokenizer=None, constraints=None, consensus=None, diversity=None, guidance=None):
        """Beam search over the dense decoder, the definition of lc_nic.NIC.beam_search (the reference only sketches
        it): log-probability beam search of width ``beam_width`` with greedy_predict's step, whose Keras mask rule it
        keeps (a 0 fed back masks the next LSTM step); at step 0 the k beams of a sample are copies and only beam 0
        counts; a beam that emits ``end_id`` (-1: never) is finished and pads with 0.  ``length_penalty`` > 0 reorders
        the k results by score / ((5 + L) / 6) ** length_penalty (model_base.length_normalise).
        The encoder and the feature step run once on the B rows; their state is gathered to the B*k beam rows.  Then
        per token: Embedding gather, input projection, LSTM step, head GEMM, softmax, and one tnt_beam_step_f32 launch
        (expansion + reorder of the state by parent into the other state buffer).  The loop is captured and replayed
        like greedy_predict, over static buffers of its own per (B, k, max_len, end_id); the paths are back-tracked on
        the host from one copy of the parents / tokens.
        ``constraints``, ``consensus``, ``diversity``, ``guidance``: model_base.DecodeConstraints, Consensus, BeamDiversity
        and Guidance, whose docstrings define them.  Here the expansion on the mixed rows of consensus or guidance is
        tnt_beam_step_f32 with U = 0 (no fused reorder), the state being gathered by the spread parents, and with
        diversity tnt_beam_step_diverse_f32 takes tnt_beam_step_f32's place on the same arguments.  With consensus the
        inputs hold G * M rows, member-major, start_seq M entries, and sequences and scores are per image: (M, k,
        max_len), (M, k).
        Returns (sequences (B, k, max_len) int64, best first; scores (B, k) float32 = sum of log-probabilities, or the
        length-normalised key)."""
        k, max_len, end_id, length_penalty = check_beam(beam_width, max_len, end_id, length_penalty, self.V)
        be, a = self.be, self.arena
        # M captions: the expansion runs on M * k rows; B = G * M staged scans: the decoder runs B * k rows, [G][M][k]
        cons, (img_input, a0, c0), start, M, G, B, con, div, ckey = self._decode_setup(
            guidance, consensus, constraints, diversity, img_input, a0, c0, start_seq, max_len, k, end_id)
        cap = torch.zeros(B, 1, dtype=torch.int32, device=self.device)
        self._stage_inputs((img_input, cap, a0, c0))
        U, E, V, ldV = self.U, self.E, self.V, self.ldV
        Bk = B * k
        key = (B, k, max_len, end_id) if cons is None else (B, k, max_len, end_id, G)
        bufs = self._beam_bufs
        if key not in bufs:
            dev, i32, f = self.device, torch.int32, self._f
            bufs[key] = dict(
                rep=torch.arange(B, dtype=i32, device=dev).repeat_interleave(k).view(Bk, 1),
                start=torch.zeros(Bk, 1, dtype=i32, device=dev),
                h=f(2, Bk, U), c=f(2, Bk, U), emb=f(Bk, E), xz=f(Bk, U, 4), out=f(Bk, U), gates=f(Bk, U, 4),
                probs=f(Bk, ldV))
        bb = bufs[key]
        bb["start"].copy_(start.repeat_interleave(k).view(Bk, 1))
        h, c, emb, xz, out, probs = bb["h"], bb["c"], bb["emb"], bb["xz"], bb["out"], bb["probs"]
        # the expansion launch: tnt_beam_step_f32, or with diversity tnt_beam_step_diverse_f32 on the same arguments.  It
        # also carries the surviving beams' state (h[1], c[1] by parent) back into h[0], c[0]; not on the mixed rows of a
        # member helper (U = 0), whose member rows gather their state by their own parent rows
        fused = cons is None
        state = (h[1], c[1], U, U, h[0], c[0]) if fused else (None, None, 0, 0, None, None)
        launch, tail = (be.beam_step, state) if div is None else (be.beam_step_diverse, state + div)
        expand = lambda p, score_in, fin_in, *outs: launch(p, ldV, score_in, fin_in, M, V, k, end_id, *outs, *tail)
        beam = _BeamDecode(self, M, k, max_len, end_id, expand, con, cons, div, bb)

        def run():
            self._decode_encode(B)
            # the B rows' state after the feature step -> the B*k beam rows (row gather b*k + j <- b)
            be.embedding_fwd(self.Hs[1], bb["rep"], h[0], Bk, 1, U, U, B)
            be.embedding_fwd(self.Cs[1], bb["rep"], c[0], Bk, 1, U, U, B)
            words = bb["start"]
            for i in range(max_len):
                self._text_step(words, i == 0, Bk, emb, xz, h[0], c[0], h[1], c[1], out, bb["gates"])
                self.gemm_sk(out, a.p("time_distributed_softmax/kernel"), probs, Bk, V, U, U, ldV, ldV,
                             bias=a.p("time_distributed_softmax/bias"))
                words, par = beam.step(i, probs)
                if not fused:
                    be.embedding_fwd(h[1], par, h[0], Bk, 1, U, U, Bk)
                    be.embedding_fwd(c[1], par, c[0], Bk, 1, U, U, Bk)
        self._run_captured(("beam",) + key + ckey, run)
        return beam.finish(length_penalty)
