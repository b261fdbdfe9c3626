"""lc_NIC -- region-wise encoder + additive attention + LSTM decoder (BASELINE config 3).

Drop-in for ``AttemptFour/Model/lc_NIC.py`` (class NIC, lines 36-838): same 17 positional
constructor arguments (lc_NIC.py:42; call site main.py:113-132), ``call`` =
``call_attention`` (223-263), ``train_step`` (328-408), ``test_step`` (410-459),
``greedy_predict`` = ``greedy_predict_attention`` (577-638).  ``groups`` is the
``(list_of_index_arrays, list_of_out_dims)`` pair of load_avg_betas.get_groups
(load_avg_betas.py:96-114).

Launch plan of one train step (hipGraph-captured):
  encoder : [dropout] -> ONE locally-dense launch (R regions) -> BatchNorm over (B,R) -> [dropout]
  hoisted : embedding gather -> [dropouts] -> text half of the LSTM input projection for all T
            steps in one GEMM; P = LeakyReLU(W1 F + b1) once (the reference recomputes it T times)
  T steps : fused attention step kernel -> fused LSTM step kernel (recurrent + context matmul + gates)
  head    : [dropout] -> Dense(256, LeakyReLU) GEMM -> [dropout] -> vocab GEMM -> softmax/CE/dlogits
  backward: mirror image; the T-step chain is lstm_step_bwd -> (dZ Wc^T) GEMM -> attention_step_bwd
  update  : [all-reduce] -> per-variable norms -> clip + Adam over the flat arena
"""
from collections import OrderedDict

import numpy as np
import torch

from . import compat
from .arena import ParamArena
from .model_base import (ModelBase, Metrics, _r4, S_IN, S_FEAT, S_TEXT, S_OUT, S_ATTN, S_LSTM_IN, S_LSTM_OUT, S_SS_COIN,
                         S_SS_DRAW, BN_EPS, BN_MOMENTUM, ScheduledSampling, check_sampling, check_length_penalty,
                         _TokenChoice, _BeamDecode, AttentionCoverage, StepRoute, LearnedInitState)

SUBJ_SITE = 1000      # dropout-site offset per subject (multi-subject model)
S_FEAT2 = 4           # second application of the feature dropout (ms2_NIC.py:214)
S_DEEP = 6            # + i: feature dropout behind deep stage i of the depth-n encoder (deep_layers.py:58)
S_NOUT = 144          # + i: output Dropout of step i of the free-running decoder, on the U-wide LSTM output (lc_NIC.py:207)
from .ops import ACT_LEAKY, attention_coverage_work_floats


def synthetic_groups(n_voxels, n_regions, out_dim, seed=42, overlap=0.0):
    """Pseudo-Glasser parcellation for benchmarks: a partition of the voxel axis into
    ``n_regions`` ragged groups (sizes log-normal, min 8, mean ~ n_voxels/n_regions), optionally
    with a fraction of extra overlapping indices.  Returns the reference's ``groups`` pair."""
    rng = np.random.default_rng(seed)
    w = rng.lognormal(0.0, 0.6, n_regions)
    sizes = np.maximum(8, np.floor(w / w.sum() * (n_voxels - 8 * n_regions)).astype(np.int64) + 8)
    while sizes.sum() > n_voxels:
        sizes[np.argmax(sizes)] -= 1
    sizes[np.argmin(sizes)] += n_voxels - sizes.sum()
    perm = rng.permutation(n_voxels)
    cuts = np.cumsum(sizes)[:-1]
    groups = [np.sort(g) for g in np.split(perm, cuts)]
    if overlap > 0:
        groups = [np.unique(np.concatenate([g, rng.choice(n_voxels, max(1, int(overlap * len(g))))])) for g in groups]
    return groups, [out_dim] * n_regions


def compact_groups(groups):
    """Input-pipeline helper for full-cortex widths: the region-wise encoder only ever reads the voxel
    columns its groups reference (after ``select_groups``, main.py:115, a good part of the 327 684-wide betas is
    unused).  Returns ``(used, groups2)``: ``used`` = sorted unique referenced columns, ``groups2`` = the same groups
    re-indexed into ``betas[:, used]``.  A generator that keeps / loads only ``betas[:, used]`` ships that many
    fewer bytes over PCIe per batch; the model built on ``groups2`` computes exactly the same function."""
    in_groups, out_groups = groups
    used = np.unique(np.concatenate([np.asarray(g, dtype=np.int64) for g in in_groups]))
    remap = np.full(int(used.max()) + 1, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return used, ([remap[np.asarray(g, dtype=np.int64)] for g in in_groups], list(out_groups))


class NIC(ModelBase):
    H = 256     # dense_inter width, hard-coded at lc_NIC.py:141
    PIECE = 64  # voxels per encoder workgroup (split mode)
    # ---- A/B switches of this model (ModelBase declares the shared ones; same rules)
    use_lc_seq = True           # False: the per-step attention / LSTM launches instead of the forward chain; INTEGRATION.md 4, tests/test_gpu_fullsize.py
    use_lc_seq_bwd = True       # False: the same for the backward chain; INTEGRATION.md 4
    branch_streams = False      # True (with use_side_streams): text and front branch of the backward in parallel; tools/probe/branch_ab.py
    split_encoder = True        # False: one workgroup per region instead of 64-voxel pieces; tools/probe/ld_split_ab.py
    voxel_major = True          # False: the split encoder reads the batch-major betas; a tool sets it by name (tools/ab_bench_att.py voxel_major=0)
    SUPPORTS_INPUT_CORRUPTION = True    # scan_dropout= / word_dropout= (ModelBase._stage_batch(corrupt=True))
    SUPPORTS_GRAD_ACCUMULATION = True   # gradient_accumulation_steps= (ModelBase._train_step_accum)
    SUPPORTS_DISTILLATION = True        # CategoricalCrossentropy(distillation=) / set_teacher (ModelBase._teach)
    # what train_step checks (compat)
    STEP_FEATURES = ("free_running", "scheduled_sampling", "attention_coverage", "init_state", "corruption")

    def __init__(self, groups, units, embedding_features, embedding_text, attn_units, vocab_size, max_length,
                 dropout_input, dropout_features, dropout_text, dropout_attn, dropout_lstm, dropout_out, input_reg,
                 attn_reg, lstm_reg, output_reg, norm="batch", n_subjects=1, depth=0, use_layer_norm=False,
                 teacher_forcing=True, scheduled_sampling=None, attention_coverage=None, scan_dropout=None,
                 word_dropout=None, init_state=None, **kw):
        super().__init__(**kw)
        # init_state (model_base.LearnedInitState): the decoder starts from h0 = tanh(mean_r(F) Wh + bh), c0 likewise, two
        # layers of its own (hidden_init, carry_init; tnt_init_state_fwd_f32 at the end of _encode); None builds nothing, and
        # the arena, the launches and every bit are those of the model without the argument
        if init_state is not None and not isinstance(init_state, LearnedInitState):
            raise ValueError(f"init_state must be None or a model_base.LearnedInitState, got {init_state!r}")
        self.init_state = init_state
        # ---- what exists only once a step or a decode has asked for it
        self.lc_xch = None              # exchange space of the persistent backward chain (_build)
        self.ew = None                  # train_step_sam's weight offset e(w)
        self._att_fb = None             # (scratch, shape) of the fused attention front backward (_bwd_front)
        self._dec_s = {}                # the decodes' attention-score buffers per (B, max_len)
        # attention_coverage (model_base.AttentionCoverage): train_step differentiates CE + L2 + weight * coverage and the
        # steps report ``coverage`` (_coverage_launch); None or weight 0 builds nothing and issues no launch
        if attention_coverage is not None and not isinstance(attention_coverage, AttentionCoverage):
            raise ValueError(f"attention_coverage must be None or a model_base.AttentionCoverage, got {attention_coverage!r}")
        self.attention_coverage = attention_coverage if attention_coverage is not None and attention_coverage.weight > 0 else None
        # teacher_forcing=False: __call__ / train_step / test_step / fit run lc_NIC.call_naive_attention (lc_NIC.py:175-221),
        # the decoder fed its own greedy predictions (call_naive_attention's docstring)
        self.teacher_forcing = bool(teacher_forcing)
        # use_layer_norm: the decoder cell is tensorflow_addons' LayerNormLSTMCell (lc_NIC.py:115,126-136; hard-wired off in
        # the reference): LayerNorm on x W, on h U and on the new cell state, no dropout inside the cell
        self.use_layer_norm = bool(use_layer_norm)
        # depth > 0: deep_layers.LocallyDense(groups, dropout, depth=n) (AttemptFour/Model/deep_layers.py:15-75) in place
        # of layers.LocallyDense -- n more stages of {per-region Dense(D -> D), BatchNorm, Dropout} behind the first one
        self.depth = int(depth)
        if self.depth and int(n_subjects) != 1:
            raise ValueError("the depth-n encoder is a single-subject variant")
        if not 0 <= self.depth < 10:
            raise ValueError("encoder depth must be in 0..9")
        # n_subjects > 1: AttemptFour/Model/ms2_NIC.py generalised to S subjects -- one region-wise
        # encoder (+ its own BatchNorm) per subject on S equal batch slices, shared decoder.
        self.S = int(n_subjects)
        self.enc_name = (lambda q: "dense_in") if self.S == 1 else (lambda q: f"dense_in_{q}")
        self.bn_name = (lambda q: "input_bn") if self.S == 1 else (lambda q: f"input_bn_{q}")
        in_groups, out_groups = groups
        assert len(in_groups) == len(out_groups), "Input groups don't match ouput groups"   # layers.py:30
        self.groups = [np.asarray(g, dtype=np.int64) for g in in_groups]
        self.R = len(self.groups)
        self.D = int(out_groups[0])
        if any(int(d) != self.D for d in out_groups):
            raise ValueError("all regions must project to the same width (they are stacked, layers.py:47-48)")
        self.U, self.Et, self.A, self.V, self.max_length = int(units), int(embedding_text), int(attn_units), int(vocab_size), int(max_length)
        self.embedding_features = embedding_features
        self.r_in, self.r_feat, self.r_text = float(dropout_input), float(dropout_features), float(dropout_text)
        self.r_attn, self.r_lstm, self.r_out = float(dropout_attn), float(dropout_lstm), float(dropout_out)
        self.l2_in, self.l2_attn, self.l2_lstm, self.l2_out = float(input_reg), float(attn_reg), float(lstm_reg), float(output_reg)
        assert norm in ("batch", "layer")
        self.norm = norm
        if self.U % 16 or self.D % 16 or self.D > 64 or self.A > 64:
            raise ValueError("kernel tiles need units % 16 == 0, group_size % 16 == 0 and <= 64, attn_units <= 64")
        R, D, A, U, Et, V, H = self.R, self.D, self.A, self.U, self.Et, self.V, self.H
        self.ldV = _r4(V)
        self.n_in = int(max(int(g.max()) for g in self.groups if len(g)) + 1)
        self.goff_host = np.concatenate([[0], np.cumsum([len(g) for g in self.groups])]).astype(np.int32)
        self.goff = torch.tensor(self.goff_host, dtype=torch.int32, device=self.device)
        # pieces of at most PIECE voxels per workgroup of the encoder kernels: one large region (Glasser regions span
        # 8..400+ voxels) would otherwise set the kernel time (tnt_locally_dense_*_split_f32)
        vg, vr, vf, rf = [0], [], [], [0]
        for r in range(self.R):
            g0, g1 = int(self.goff_host[r]), int(self.goff_host[r + 1])
            k = g0
            while True:
                k2 = min(g1, k + self.PIECE)
                vg.append(k2); vr.append(r); vf.append(1 if k == g0 else 0)
                k = k2
                if k >= g1:
                    break
            rf.append(len(vr))
        ti = lambda a: torch.tensor(a, dtype=torch.int32, device=self.device)
        self.vgoff, self.vreg, self.vfirst, self.rfirst, self.NV = ti(vg), ti(vr), ti(vf), ti(rf), len(vr)
        self.idx = torch.tensor(np.concatenate(self.groups).astype(np.int32), dtype=torch.int32, device=self.device)
        ls = OrderedDict()
        ks = OrderedDict()
        for q in range(self.S):
            en, bn = self.enc_name(q), self.bn_name(q)
            for r, g in enumerate(self.groups):
                ls[f"{en}/{r}"] = ["kernel", "bias"]
                ks[f"{en}/{r}/kernel"] = (len(g), D)
                ks[f"{en}/{r}/bias"] = (D,)
            ls[bn] = ["gamma", "beta", "moving_mean", "moving_variance"]
            for w in ls[bn]:
                ks[f"{bn}/{w}"] = (D,)
        for i in range(self.depth):
            for r in range(self.R):
                ls[f"dense_in/deep{i}/{r}"] = ["kernel", "bias"]
                ks[f"dense_in/deep{i}/{r}/kernel"], ks[f"dense_in/deep{i}/{r}/bias"] = (D, D), (D,)
            ls[f"input_bn/deep{i}"] = ["gamma", "beta", "moving_mean", "moving_variance"]
            for w in ls[f"input_bn/deep{i}"]:
                ks[f"input_bn/deep{i}/{w}"] = (D,)
        for nm, shp in (("attention/W1", (D, A)), ("attention/W2", (U, A)), ("attention/V", (A, 1))):
            ls[nm] = ["kernel", "bias"]
            ks[f"{nm}/kernel"] = shp
            ks[f"{nm}/bias"] = (shp[1],)
        ls["emb_text"] = ["embeddings"]
        ks["emb_text/embeddings"] = (V, Et)
        ls["lstm"] = ["kernel", "recurrent_kernel", "bias"]
        ks["lstm/kernel"], ks["lstm/recurrent_kernel"], ks["lstm/bias"] = (D + Et, 4 * U), (U, 4 * U), (4 * U,)
        if self.use_layer_norm:
            for nm, n in (("kernel_norm", 4 * U), ("recurrent_norm", 4 * U), ("state_norm", U)):
                ls[f"lstm/{nm}"] = ["gamma", "beta"]
                ks[f"lstm/{nm}/gamma"], ks[f"lstm/{nm}/beta"] = (n,), (n,)
        ls["time_distributed_nonlinear"] = ["kernel", "bias"]
        ks["time_distributed_nonlinear/kernel"], ks["time_distributed_nonlinear/bias"] = (U, H), (H,)
        ls["time_distributed_softmax"] = ["kernel", "bias"]
        ks["time_distributed_softmax/kernel"], ks["time_distributed_softmax/bias"] = (H, V), (V,)
        if self.init_state is not None:
            for nm in LearnedInitState.LAYERS:
                ls[nm] = ["kernel", "bias"]
                ks[f"{nm}/kernel"], ks[f"{nm}/bias"] = (D, U), (U,)
        self.layers_spec, self.keras_shapes = ls, ks

        a = self.arena = ParamArena(self.device)
        enc_off = []
        for q in range(self.S):
            en, bn = self.enc_name(q), self.bn_name(q)
            for r, g in enumerate(self.groups):                  # contiguous CSR concatenation
                a.add(f"{en}/{r}/kernel", (len(g), D), self.l2_in, align=4)
            w_off = a.entries[f"{en}/0/kernel"].off
            a.total = (a.total + 63) // 64 * 64
            for r in range(R):
                a.add(f"{en}/{r}/bias", (D,), align=4)
            enc_off.append((w_off, a.entries[f"{en}/0/bias"].off))
            a.total = (a.total + 63) // 64 * 64
            a.add(f"{bn}/gamma", (D,)); a.add(f"{bn}/beta", (D,))
        deep_off = []
        for i in range(self.depth):
            for r in range(R):
                a.add(f"dense_in/deep{i}/{r}/kernel", (D, D), self.l2_in, align=4)
            w_off = a.entries[f"dense_in/deep{i}/0/kernel"].off
            a.total = (a.total + 63) // 64 * 64
            for r in range(R):
                a.add(f"dense_in/deep{i}/{r}/bias", (D,), align=4)
            deep_off.append((w_off, a.entries[f"dense_in/deep{i}/0/bias"].off))
            a.total = (a.total + 63) // 64 * 64
            a.add(f"input_bn/deep{i}/gamma", (D,)); a.add(f"input_bn/deep{i}/beta", (D,))
        a.add("attention/W1/kernel", (D, A), self.l2_attn); a.add("attention/W1/bias", (A,))
        a.add("attention/W2/kernel", (U, A), self.l2_attn); a.add("attention/W2/bias", (A,))
        a.add("attention/V/kernel", (A,)); a.add("attention/V/bias", (1,))
        a.add("emb_text/embeddings", (V, Et))
        a.add("lstm/kernel", (D + Et, U, 4), self.l2_lstm)
        a.add("lstm/recurrent_kernel", (U, U, 4)); a.add("lstm/bias", (U, 4))
        if self.use_layer_norm:
            for nm in ("kernel_norm", "recurrent_norm"):
                a.add(f"lstm/{nm}/gamma", (U, 4)); a.add(f"lstm/{nm}/beta", (U, 4))
            a.add("lstm/state_norm/gamma", (U,)); a.add("lstm/state_norm/beta", (U,))
        a.add("time_distributed_nonlinear/kernel", (U, H), self.l2_out); a.add("time_distributed_nonlinear/bias", (H,))
        a.add("time_distributed_softmax/kernel", (H, self.ldV), self.l2_out)
        a.add("time_distributed_softmax/bias", (self.ldV,))
        if self.init_state is not None:         # behind every entry of the model without them
            for nm in LearnedInitState.LAYERS:
                a.add(f"{nm}/kernel", (D, U), self.init_state.reg); a.add(f"{nm}/bias", (U,))
        a.finalize()
        nW = int(self.goff_host[-1]) * D
        self.encW = [a.theta[w:w + nW] for w, _ in enc_off]
        self.encWg = [a.grad[w:w + nW] for w, _ in enc_off]
        self.encB = [a.theta[b:b + R * D] for _, b in enc_off]
        self.encBg = [a.grad[b:b + R * D] for _, b in enc_off]
        self.deepW = [a.theta[w:w + R * D * D] for w, _ in deep_off]
        self.deepWg = [a.grad[w:w + R * D * D] for w, _ in deep_off]
        self.deepB = [a.theta[b:b + R * D] for _, b in deep_off]
        self.deepBg = [a.grad[b:b + R * D] for _, b in deep_off]
        self.deep_idx = torch.arange(R * D, dtype=torch.int32, device=self.device)
        self.deep_goff = torch.arange(0, (R + 1) * D, D, dtype=torch.int32, device=self.device)
        # moving statistics: one pair per subject encoder, then one pair per deep stage
        self.mov_mean = [self._f(D) for _ in range(self.S + self.depth)]
        self.mov_var = [torch.ones(D, dtype=torch.float32, device=self.device) for _ in range(self.S + self.depth)]
        self.drop_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        # scheduled_sampling (model_base.ScheduledSampling): train_step feeds each caption row the model's own token with the
        # schedule's probability (tnt_scheduled_feedback2_f32, _forward_ss); None keeps the teacher-forced step
        self.scheduled_sampling = scheduled_sampling
        if scheduled_sampling is not None:
            self._ss_check()
            self.ss_sched = torch.tensor(scheduled_sampling.params(), dtype=torch.float64, device=self.device)
        self._init_weights(np.random.default_rng(self.seed))
        self._shape = None
        if not self.teacher_forcing:
            self._naive_check()
        compat.check(self, ("scheduled_sampling", "free_running", "attention_coverage", "init_state"))
        # scan_dropout (model_base.ScanDropout) / word_dropout (model_base.WordDropout): train_step and train_step_sam corrupt
        # the staged batch (tnt_input_corrupt_f32, one launch behind the staging); None or rate 0 issues nothing
        self.scan_dropout, self.word_dropout = scan_dropout, word_dropout

    def _input_width(self):
        return self.n_in

    # ------------------------------------------------------------------ weights
    def _init_weights(self, rng):
        """Initialisers of lc_NIC.py:84-159 / attention.py:21-23."""
        D, A, U, Et, V, H = self.D, self.A, self.U, self.Et, self.V, self.H
        tn = lambda shape, std: np.clip(rng.standard_normal(shape), -2, 2) * std / 0.8796
        for q in range(self.S):
            for r, g in enumerate(self.groups):
                self.set_weight(f"{self.enc_name(q)}/{r}/kernel", tn((len(g), D), np.sqrt(2.0 / max(len(g), 1))))  # he_normal
            self.set_weight(f"{self.bn_name(q)}/gamma", np.ones(D))
        for i in range(self.depth):
            for r in range(self.R):
                self.set_weight(f"dense_in/deep{i}/{r}/kernel", tn((D, D), np.sqrt(2.0 / D)))
            self.set_weight(f"input_bn/deep{i}/gamma", np.ones(D))
        self.set_weight("attention/W1/kernel", tn((D, A), np.sqrt(2.0 / D)))
        self.set_weight("attention/W2/kernel", tn((U, A), np.sqrt(2.0 / U)))
        lim = np.sqrt(6.0 / (A + 1))
        self.set_weight("attention/V/kernel", rng.uniform(-lim, lim, (A, 1)))
        self.set_weight("emb_text/embeddings", rng.uniform(-0.08, 0.08, (V, Et)))
        lim = np.sqrt(6.0 / (D + Et + 4 * U))
        self.set_weight("lstm/kernel", rng.uniform(-lim, lim, (D + Et, 4 * U)))
        q = np.concatenate([np.linalg.qr(rng.standard_normal((U, U)))[0] for _ in range(4)], axis=1)
        self.set_weight("lstm/recurrent_kernel", q)
        b = np.zeros(4 * U); b[U:2 * U] = 1.0
        self.set_weight("lstm/bias", b)
        if self.use_layer_norm:
            for nm, n in (("kernel_norm", 4 * U), ("recurrent_norm", 4 * U), ("state_norm", U)):
                self.set_weight(f"lstm/{nm}/gamma", np.ones(n))
        self.set_weight("time_distributed_nonlinear/kernel", tn((U, H), np.sqrt(2.0 / (U + H))))
        self.set_weight("time_distributed_softmax/kernel", tn((H, V), np.sqrt(2.0 / (H + V))))
        if self.init_state is not None:         # glorot_uniform, drawn behind every other weight: those keep their values
            lim = np.sqrt(6.0 / (D + U))
            for nm in LearnedInitState.LAYERS:
                self.set_weight(f"{nm}/kernel", rng.uniform(-lim, lim, (D, U)))

    def _bn_slots(self):
        """(slot of mov_mean / mov_var, keras layer name) of every BatchNormalization of the encoder"""
        return [(q, self.bn_name(q)) for q in range(self.S)] + [(self.S + i, f"input_bn/deep{i}") for i in range(self.depth)]

    def _state_map(self):
        slots = self._bn_slots()        # every moving mean, then every moving variance
        return OrderedDict([(f"{bn}/moving_mean", self.mov_mean[q]) for q, bn in slots]
                           + [(f"{bn}/moving_variance", self.mov_var[q]) for q, bn in slots])

    # ------------------------------------------------------------------ buffers
    def _build(self, B, T):
        if self._shape == (B, T):
            return
        if B % self.S:
            raise ValueError("batch must split into n_subjects equal slices")
        f = self._f
        R, D, A, U, Et, V, H, ldV = self.R, self.D, self.A, self.U, self.Et, self.V, self.H, self.ldV
        n = T * B
        self.ldx = _r4(self.n_in)
        self.x = f(B, self.ldx)
        self.xd = f(B, self.ldx) if self.r_in > 0 else self.x
        self.cap = torch.zeros(B, T, dtype=torch.int32, device=self.device)
        self.tgt = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.enc_pre, self.enc_y = f(B, R, D), f(B, R, D)
        self.enc_part = f(self.NV, 64, D)                    # piece partials of the split encoder forward
        self.dctx_part = f(U // 16, B, D)                    # per-unit-block context-gradient partials of a BPTT step
        # voxel-major copy of the betas for the encoder's gather (a voxel's batch values contiguous); not with input
        # dropout, whose mask is defined on the batch-major tensor
        self.xT = f(self.n_in, (B + 3) // 4 * 4) if (self.r_in == 0 and self.ldx == self.n_in) else None
        self.xhat, self.inv_std = f(B * R, D), f(self.S, max(B * R, D))
        # depth-n encoder: stage i reads Fs[i] and writes Fs[i + 1]; the attention reads the last one
        self.Fs = [f(B, R, D) for _ in range(self.depth + 1)]
        self.F = self.Fs[-1]
        self.deep_pre = [f(B, R, D) for _ in range(self.depth)]
        self.deep_y = [f(B, R, D) for _ in range(self.depth)]
        self.deep_xhat = [f(B * R, D) for _ in range(self.depth)]
        self.deep_istd = [f(max(B * R, D)) for _ in range(self.depth)]
        self.dFd = f(B, R, D) if self.depth else None
        self.text = f(n, Et)
        self.XZ = f(n, U, 4)
        self.P, self.Ppre = f(B * R, A), f(B * R, A)
        self.Hs, self.Cs = f(T + 1, B, U), f(T + 1, B, U)
        self.gates = f(T, B, U, 4)
        self.qpre, self.alpha = f(T, B, A), f(T, B, R)
        self.ctx, self.ctx_d = f(T, B, D), f(T, B, D)
        self.Hd = f(n, U) if (self.r_lstm > 0 or self.r_out > 0) else None
        self.last_ids = torch.zeros(B, dtype=torch.int32, device=self.device)     # free-running decode: step T-1's argmax
        if self.use_layer_norm:       # LayerNormLSTMCell: normalised projections, LayerNorm caches, per-step gradients
            self.ZK, self.ZR, self.ZRn = f(n, U, 4), f(n, U, 4), f(n, U, 4)
            self.xh_k, self.xh_r = f(n, 4 * U), f(n, 4 * U)
            self.is_k, self.is_r, self.is_s = f(T, max(B, 4 * U)), f(T, max(B, 4 * U)), f(T, B)
            self.chat, self.dcnt = f(n, U), f(n, U)
            self.dZK, self.dZR = f(n, U, 4), f(n, U, 4)
            self.dh_rec = f(B, U)
        self.ipre, self.inter = f(n, H), f(n, H)
        self.inter_d = f(n, H) if self.r_out > 0 else self.inter
        self.logits = f(n, ldV)
        self.loss_row, self.corr_row = f(n), f(n)
        self.met = f(8 + 4 * self.S)
        self._init_seq_lstm(B, U)        # device census + sync state of the persistent chain kernels (tnt_lc_seq_{fwd,bwd}_f32)
        self.lc_xch = None                # exchange space of the persistent backward chain
        if self._seq_lstm and hasattr(self.be, "lc_seq_bwd") and B <= 128:
            self.lc_xch = f(self.be.lc_seq_bwd_work_floats(B, U))
        if self._seq_lstm and hasattr(self.be, "lc_seq_fwd") and B <= 128:
            self.lc_fwd_work = f(self.be.lc_seq_fwd_work_floats(B))
        self.colB = f(2 * B)
        # backward
        self.dinter, self.dHs = f(n, H), f(n, U)
        self.dZ = f(n, U, 4)
        self.dc, self.dh_att = f(B, U), f(B, U)
        self.dctx = f(B, D)
        # the three accumulators of the attention backward sit in one allocation: one fill zeroes them per step
        pad4 = lambda v: -(-v // 4) * 4                      # every piece starts 16-byte aligned
        oF, ovb = pad4(B * R * A), pad4(B * R * A) + pad4(B * R * D)
        self.datt = f(ovb + pad4(B * (A + 1)))
        self.dP, self.dF = self.datt[:B * R * A].view(B * R, A), self.datt[oF:oF + B * R * D].view(B, R, D)
        self.dvb, self.dqpre = self.datt[ovb:ovb + B * (A + 1)].view(B, A + 1), f(T, B, A)
        # attention-dropout keep bits of all T timesteps (4 per byte), produced by ONE chip-wide launch per step instead
        # of Philox inside every per-timestep kernel on the serial chain (2 us forward + 2.4 us backward per timestep)
        self._keep_stored = self.r_attn > 0 and A % 4 == 0
        self.att_keep = (torch.zeros(T, B * R * A // 4, dtype=torch.uint8, device=self.device)
                         if self._keep_stored else None)
        self.dtext = f(n, Et)
        self.dbn = f(B * R, D)
        nch = max(self.be.bn_nchunk(B * R), self.be.bn_nchunk(n))
        self.work = f(max(D, A, 4 * U, ldV, H) * (2 * nch + 1))
        self.rowsq = f(n)
        self.metric_part = f(T * ((self.R + 63) // 64))      # partial sums of the attention metric (tnt_attention_metric_parts)
        if self.init_state is not None:     # the region means the init backward reads, and the gradients of the two states
            self.fmean, self.dh0, self.dc0 = f(B, D), f(B, U), f(B, U)
        cov = self.attention_coverage
        if cov is not None:     # the coverage gradient rider [rows][R] and the partials of the value (tnt_attention_coverage_f32)
            self.cov_ext = f(cov.rows(T, B) * R)
            self.cov_work = f(attention_coverage_work_floats(T, B, R, cov.axis_id))
        self._alloc_splitk([(n, H, V), (n, Et, 4 * U), (n, U, H), (D, 4 * U, n), (U, A, n), (D, A, B * R)])
        self.emb_seg = self.arena.entries["emb_text/embeddings"].seg
        self._shape = (B, T)
        self._graphs = {}
        if self.optimizer is not None and self.opt_m is None:
            self._init_optimizer_state()
        self.built = True

    def _stage_inputs(self, data):
        self._route = StepRoute()
        x, cap, a0, c0 = data[:4]
        cap_t = self._to_dev(cap, torch.int32)
        if cap_t.dim() == 1:
            cap_t = cap_t.view(-1, 1)
        B, T = cap_t.shape
        self._build(B, T)
        xs = self._to_dev(x, torch.float32)
        assert xs.shape[0] == B and xs.shape[1] >= self.n_in, f"betas shape {tuple(xs.shape)}"
        self.x[:, :self.n_in].copy_(xs[:, :self.n_in])
        if self.xT is not None:
            self.xT[:, :B].copy_(self.x[:, :self.n_in].t())
        self.cap.copy_(cap_t)
        # (with init_state the two copies are shape checks only: _encode overwrites slab 0 with the learned state)
        self.Hs[0].copy_(self._to_dev(a0, torch.float32))
        self.Cs[0].copy_(self._to_dev(c0, torch.float32))
        return B, T

    # ------------------------------------------------------------------ forward
    def _encode(self, B, training, feat2=False):
        """dropout_input -> layers.LocallyDense.call (lc_NIC.py:227-230; layers.py:43-53).  feat2: the feature Dropout
        once more behind the encoder (call_naive_attention, lc_NIC.py:183-184)."""
        be, a = self.be, self.arena
        R, D, S = self.R, self.D, self.S
        sd, ds = self.seed, self.drop_step
        Bs = B // S
        for q in range(S):                       # one encoder per subject on its batch slice (ms2_NIC.py:181-203)
            off = SUBJ_SITE * (q + 1) if S > 1 else 0
            r0, r1 = q * Bs, (q + 1) * Bs
            x = self.x[r0:r1]
            if training and self.r_in > 0:
                be.dropout(x, self.xd[r0:r1], Bs, self.n_in, self.ldx, 0, self.n_in, 0, self.r_in, sd, S_IN + off, 0, ds)
                x = self.xd[r0:r1]
            if self.NV > R and hasattr(be, "locally_dense_fwd_split") and self.split_encoder:
                vm = self.xT is not None and self.voxel_major
                be.locally_dense_fwd_split(self.xT[:, r0:r1] if vm else x, self.xT.shape[1] if vm else self.ldx, self.idx,
                                           self.vgoff, self.vreg, self.rfirst, self.NV, self.encW[q], self.encB[q],
                                           self.enc_pre[r0:r1], self.enc_y[r0:r1], self.enc_part, Bs, R, D, 0.2,
                                           voxel_major=vm)
            else:
                be.locally_dense_fwd(x, self.ldx, self.idx, self.goff, self.encW[q], self.encB[q],
                                     self.enc_pre[r0:r1], self.enc_y[r0:r1], Bs, R, D, 0.2)
            bn = self.bn_name(q)
            Fq, xh = self.Fs[0][r0:r1], self.xhat[r0 * R:r1 * R]
            dropped = False
            if self.norm == "batch":                 # the feature Dropout (layers.py:51) rides in the BN apply pass
                drop = (self.r_feat, sd, S_FEAT + off, ds) if training and self.r_feat > 0 else None
                dropped = self._bn_fwd(self.enc_y[r0:r1], a.p(f"{bn}/gamma"), a.p(f"{bn}/beta"), self.mov_mean[q],
                                       self.mov_var[q], Fq, xh, self.inv_std[q], Bs * R, D, D, training, self.work, drop=drop)
            else:
                be.layernorm_fwd(self.enc_y[r0:r1], a.p(f"{bn}/gamma"), a.p(f"{bn}/beta"), Fq, xh, self.inv_std[q],
                                 Bs * R, D, D, BN_EPS)
            if training and self.r_feat > 0:
                if not dropped:
                    be.dropout(Fq, Fq, Bs * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT + off, 0, ds)        # layers.py:51
                if S > 1:                        # ms2_NIC.py:214,257: the feature Dropout is applied a second time
                    be.dropout(Fq, Fq, Bs * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT2 + off, 0, ds)
        for i in range(self.depth):              # deep_layers.one_layer (deep_layers.py:53-59): Dense_r(x[:, r, :]), BN, Dropout
            xin, out = self.Fs[i], self.Fs[i + 1]
            be.locally_dense_fwd(xin, R * D, self.deep_idx, self.deep_goff, self.deepW[i], self.deepB[i], self.deep_pre[i],
                                 self.deep_y[i], B, R, D, 0.2)
            bn, q = f"input_bn/deep{i}", self.S + i
            dropped = False
            if self.norm == "batch":
                drop = (self.r_feat, sd, S_DEEP + i, ds) if training and self.r_feat > 0 else None
                dropped = self._bn_fwd(self.deep_y[i], a.p(f"{bn}/gamma"), a.p(f"{bn}/beta"), self.mov_mean[q], self.mov_var[q],
                                       out, self.deep_xhat[i], self.deep_istd[i], B * R, D, D, training, self.work, drop=drop)
            else:
                be.layernorm_fwd(self.deep_y[i], a.p(f"{bn}/gamma"), a.p(f"{bn}/beta"), out, self.deep_xhat[i],
                                 self.deep_istd[i], B * R, D, D, BN_EPS)
            if training and self.r_feat > 0 and not dropped:
                be.dropout(out, out, B * R, D, D, 0, D, 0, self.r_feat, sd, S_DEEP + i, 0, ds)
        if feat2 and training and self.r_feat > 0:
            be.dropout(self.F, self.F, B * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT2, 0, ds)
        self.gemm_sk(self.F, a.p("attention/W1/kernel"), self.P, B * R, self.A, D, D, self.A, self.A,
                bias=a.p("attention/W1/bias"), pre=self.Ppre, act=ACT_LEAKY, slope=0.2)      # attention.py:32 (hoisted)
        if self.init_state is not None:
            # the learned initial state from the features the attention reads, over the staged a0 / c0 (slab 0 of Hs / Cs,
            # where both chains, the per-step kernels, the decodes and score_captions' gather read it)
            be.init_state_fwd(self.F, a.p("hidden_init/kernel"), a.p("hidden_init/bias"), a.p("carry_init/kernel"),
                              a.p("carry_init/bias"), self.fmean, self.Hs[0], self.Cs[0], B, R, D, self.U)

    def _lc_seq_ok(self):
        """the persistent forward-chain kernel applies (tnt_lc_seq_fwd_f32's shape limits; the device census was taken by
        _init_seq_lstm in _build)"""
        # Default on (use_lc_seq = False selects the two per-step launches).  MI355X, B = 64, R = 360, U = 512: the chain as one
        # launch of role-specialised workgroups (16 attention + 16 LSTM workgroups per XCD, step-invariant operands resident,
        # the recurrent product overlapped with the attention) takes config 3 from 1.010 to 0.920 ms/step
        # (tools/ab_attr.py attention use_lc_seq=False).  An earlier form that ran both phases on the same workgroups one
        # after the other was slower than the per-step launches (16.3 vs 15.6 us per step): attention and LSTM register sets
        # together spilled 58 VGPRs and half of each group idled through the attention phase.
        return bool(self._seq_lstm and self.use_lc_seq and not self.use_layer_norm
                    and hasattr(self.be, "lc_seq_fwd") and self.R <= (512 if max(self.A, self.D) <= 32 else 384)
                    and self.A % 4 == 0 and self.D % 4 == 0 and self.A <= 64 and self.D <= 64)

    def _decode_step(self, i, B, training, s_out=None, xz_bias=None):
        """attention -> concat -> one LSTM step (lc_NIC.py:246-255)."""
        be, a = self.be, self.arena
        R, D, A, U, Et = self.R, self.D, self.A, self.U, self.Et
        Wl = a.p("lstm/kernel")
        r_in = self.r_lstm if (training and not self.use_layer_norm) else 0.0      # the LayerNorm cell has no input dropout
        be.attention_step_fwd(self.Hs[i], self.F, self.P, a.p("attention/W2/kernel"), a.p("attention/W2/bias"),
                              a.p("attention/V/kernel"), a.p("attention/V/bias"), self.qpre[i], self.alpha[i],
                              self.ctx[i], self.ctx_d[i], s_out, B, R, D, A, U, 0.2,
                              self.r_attn if training else 0.0, r_in, D + Et, self.seed,
                              S_ATTN + i, S_LSTM_IN + i, 0, self.drop_step,
                              keep4=self.att_keep[i] if (training and self._keep_stored) else None)
        if self.use_layer_norm:
            # LayerNormLSTMCell.call: z = LN_kernel([ctx, text] W) + LN_recurrent(h U) + b, state LayerNorm inside the cell
            rows = slice(i * B, (i + 1) * B)
            xz = self.XZ[rows]                       # text part of x W (all T steps in one GEMM, no bias) ...
            self.gemm_sk(self.ctx_d[i], Wl[:D], xz, B, 4 * U, D, D, 4 * U, 4 * U, accumulate=True)       # ... + ctx W_ctx
            be.layernorm_fwd(xz, a.p("lstm/kernel_norm/gamma"), a.p("lstm/kernel_norm/beta"), self.ZK[rows], self.xh_k[rows],
                             self.is_k[i], B, 4 * U, 4 * U, BN_EPS)
            self.gemm_sk(self.Hs[i], a.p("lstm/recurrent_kernel"), self.ZR[rows], B, 4 * U, U, U, 4 * U, 4 * U)
            be.layernorm_fwd(self.ZR[rows], a.p("lstm/recurrent_norm/gamma"), a.p("lstm/recurrent_norm/beta"), self.ZRn[rows],
                             self.xh_r[rows], self.is_r[i], B, 4 * U, 4 * U, BN_EPS)
            be.ln_lstm_cell_fwd(self.ZK[rows], self.ZRn[rows], a.p("lstm/bias"), self.Cs[i], a.p("lstm/state_norm/gamma"),
                                a.p("lstm/state_norm/beta"), self.gates[i], self.chat[rows], self.is_s[i], self.Cs[i + 1],
                                self.Hs[i + 1], B, U, BN_EPS)
            return
        be.lstm_step_fwd(self.XZ[i * B:(i + 1) * B], self.Hs[i], self.Cs[i], a.p("lstm/recurrent_kernel"),
                         self.ctx_d[i], Wl[:D], D, None, 0, 0, None, self.Hs[i + 1], self.Cs[i + 1], None,
                         self.gates[i], B, U, xz_bias=xz_bias)

    def _token_step(self, i, words, B, logits, s_out=None):
        """this model's half of decoded token i (lc_NIC.py:596-623): the Embedding of the B fed ``words``, the text half of
        the input projection, attention -> LSTM step in inference mode, the head into ``logits``"""
        be, a = self.be, self.arena
        D, U, Et = self.D, self.U, self.Et
        rows = slice(i * B, (i + 1) * B)
        be.embedding_fwd(a.p("emb_text/embeddings"), words, self.text[rows], B, 1, Et, Et, self.V)
        self.gemm_sk(self.text[rows], a.p("lstm/kernel")[D:], self.XZ[rows], B, 4 * U, Et, Et, 4 * U, 4 * U,
                     bias=None if self.use_layer_norm else a.p("lstm/bias"))      # LN cell: bias behind the norms
        self._decode_step(i, B, False, s_out)
        self._head_inter(self.Hs[i + 1], self.inter[:B], B)
        self._head_out(self.inter[:B], logits, B)

    def _text_front(self, B, T, training, fed=None):
        """The text front of a forward pass (lc_NIC.py:233 and the Dropouts behind it): the Embedding of all T caption
        columns, the text Dropout, the text half of the per-call LSTM input mask over (B, 1, D + Et), the text half of the
        input projection into XZ (one epilogue-free GEMM; the bias is added in the step kernel), the stored attention
        keep-masks.  ``fed``: None = teacher-forced, "ss" = scheduled sampling (always training), "naive" = free-running.
        Embedding + text Dropout are one launch when training with r_text > 0 and Et % 4 == 0 (_ss_check / _naive_check
        guarantee the layout); the LSTM input mask rides in it when r_lstm > 0 -- teacher-forced only where D % 4 == 0,
        which the fed modes do not consult.  Otherwise
        the text Dropout covers all n = T*B rows, geometry (B, Et, 0), and the LSTM input mask all n rows with
        rows_per_site=B -- free-running: step 0's B rows only, without rows_per_site.  XZ is projected for all n rows
        teacher-forced, for step 0's B rows in the fed modes: their feedback launches write the later rows of ``text``
        and ``XZ``.  The keep-masks are generated here unless a training step staged them with its batch, outside the
        captured sequence (_stage_mask_job)."""
        be, a = self.be, self.arena
        D, U, Et, V = self.D, self.U, self.Et, self.V
        n = T * B
        sd, ds = self.seed, self.drop_step
        emb = a.p("emb_text/embeddings")
        lstm_in_mask = training and self.r_lstm > 0 and not self.use_layer_norm
        if training and self.r_text > 0 and Et % 4 == 0:
            ride = lstm_in_mask and (fed is not None or D % 4 == 0)
            be.embedding_fwd_drop(emb, self.cap, None, self.text, B, T, Et, Et, V, self.r_text, sd, S_TEXT, 0, ds,
                                  mask2=(self.r_lstm, S_LSTM_IN, D + Et, D) if ride else None)
            lstm_in_mask = lstm_in_mask and not ride
        else:
            be.embedding_fwd(emb, self.cap, self.text, B, T, Et, Et, V)
            if training and self.r_text > 0:
                be.dropout(self.text, self.text, n, Et, Et, B, Et, 0, self.r_text, sd, S_TEXT, 0, ds)
        if lstm_in_mask and fed == "naive":
            be.dropout(self.text, self.text, B, Et, Et, 0, D + Et, D, self.r_lstm, sd, S_LSTM_IN, 0, ds)
        elif lstm_in_mask:
            be.dropout(self.text, self.text, n, Et, Et, 0, D + Et, D, self.r_lstm, sd, S_LSTM_IN, 0, ds, rows_per_site=B)
        m = n if fed is None else B
        self.gemm_sk(self.text[:m], a.p("lstm/kernel")[D:], self.XZ[:m], m, 4 * U, Et, Et, 4 * U, 4 * U)
        if training and self._keep_stored and not self._route.masks_staged:
            be.dropout_mask4(self.att_keep, B * self.R * self.A, T, self.r_attn, sd, S_ATTN, 0, ds)

    def _head_inter(self, h, inter, n, ipre=None):
        """dense_inter over n rows (lc_NIC.py:141,258): inter = LeakyReLU(h W + b); ``ipre`` keeps the pre-activation
        for the backward pass (None: the inference form)"""
        a, U, H = self.arena, self.U, self.H
        self.gemm_sk(h, a.p("time_distributed_nonlinear/kernel"), inter, n, H, U, U, H, H,
                     bias=a.p("time_distributed_nonlinear/bias"), pre=ipre, act=ACT_LEAKY, slope=0.2)

    def _head_out(self, inter, logits, n):
        """dense_out over n rows (lc_NIC.py:261): the logits; the softmax is the caller's"""
        a, V, H, ldV = self.arena, self.V, self.H, self.ldV
        self.gemm_sk(inter, a.p("time_distributed_softmax/kernel"), logits, n, V, H, H, ldV, ldV,
                     bias=a.p("time_distributed_softmax/bias"))

    def _forward(self, B, T, training):
        be, a = self.be, self.arena
        R, D, A, U, Et, H = self.R, self.D, self.A, self.U, self.Et, self.H
        n = T * B
        sd, ds = self.seed, self.drop_step
        self._encode(B, training)
        self._text_front(B, T, training)
        Wl = a.p("lstm/kernel")
        if self._lc_seq_ok():
            # the T attention -> LSTM steps as ONE persistent launch (tnt_lc_seq_fwd_f32), XCD-local data-polling hand-offs
            r_in = self.r_lstm if training else 0.0
            keep = self.att_keep if (training and self._keep_stored) else None
            # (with the Dropout behind the LSTM, :256, as a rider of the same launch: Hd leaves the chain with hs)
            out_dropped = bool(training and self.r_lstm > 0)
            be.lc_seq_fwd(self.F, self.P, a.p("attention/W2/kernel"), a.p("attention/W2/bias"), a.p("attention/V/kernel"),
                          a.p("attention/V/bias"), self.qpre, self.alpha, self.ctx, self.ctx_d, keep,
                          B * R * A // 4 if keep is not None else 0, self.XZ, Wl[:D], a.p("lstm/recurrent_kernel"),
                          a.p("lstm/bias"), self.Hs, self.Cs, self.gates, T, B, R, D, A, U, 0.2,
                          self.r_attn if training else 0.0, r_in, D + Et, self.seed, S_ATTN, S_LSTM_IN, self.drop_step,
                          self.lc_fwd_work, self.seq_sync, self._guard_out(),
                          out_drop=(self.Hd, self.r_lstm, S_LSTM_OUT) if out_dropped else None)
        else:
            out_dropped = False
            for i in range(T):                                                                  # :244-256
                self._decode_step(i, B, training, xz_bias=a.p("lstm/bias"))
        hs = self.Hs[1:].view(n, U)
        if out_dropped:
            hs = self.Hd
        elif training and self.r_lstm > 0:                                                      # :256
            be.dropout(hs, self.Hd, n, U, U, 0, U, 0, self.r_lstm, sd, S_LSTM_OUT, 0, ds, rows_per_site=B)
            hs = self.Hd
        self._route.hs_used = hs
        self._head_inter(hs, self.inter, n, self.ipre)
        inter = self.inter
        self._tail.metric_parts_ready = False
        if training and self.r_out > 0:
            npart = be.attention_metric_parts(T, self.R) if hasattr(be, "dropout_metric") else 0
            if (self.S == 1 and self._tail.deferring and H % 4 == 0
                    and 0 < npart <= self.metric_part.numel()):
                # the attention metric's partials (:365-367) ride in this launch: alpha is complete behind the chain
                be.dropout_metric(self.inter, self.inter_d, n, H, H, B, H, 0, self.r_out, sd, S_OUT, 0, ds, self.alpha,
                                  self.metric_part, T, B, self.R)
                self._tail.metric_parts_ready = True
            else:
                be.dropout(self.inter, self.inter_d, n, H, H, B, H, 0, self.r_out, sd, S_OUT, 0, ds)
            inter = self.inter_d
        self._route.inter_used = inter
        self._head_out(inter, self.logits, n)

    def learn_init_state(self, img_input):
        """lc_NIC.learn_init_state (lc_NIC.py:169-173) on the scans ``img_input`` (B, n_voxels): (h0, c0), two (B, units)
        numpy arrays, in inference mode (moving BatchNorm statistics, no Dropout)"""
        if self.init_state is None:
            raise ValueError("learn_init_state needs a model built with init_state=model_base.LearnedInitState(...)")
        B = int(np.shape(img_input)[0])
        z = np.zeros((B, self.U), np.float32)
        self._stage_inputs((img_input, torch.zeros(B, 1, dtype=torch.int32), z, z))
        self._encode(B, False)
        return self.Hs[0].cpu().numpy().copy(), self.Cs[0].cpu().numpy().copy()

    def _bwd_init(self, B, T):
        """the backward of the learned initial state, between the chain and _bwd_front (which finishes dF: the folded
        feature Dropout' acts on the finished dF).  dh0 = dZ[0] Ur^T + dqpre[0] W2^T: two products of the dtext shape; on
        the per-step route the second is what step 0's attention backward left in dh_att, and dc what its cell backward
        left.  Then tnt_init_state_bwd_f32: the four parameter gradients (left out where both layers are frozen) and its
        share of dF."""
        if self.init_state is None:
            return
        be, a = self.be, self.arena
        R, D, A, U = self.R, self.D, self.A, self.U
        Ur = a.p("lstm/recurrent_kernel")
        if self._lc_seq_bwd_ok():
            dh0, dc0 = self.dh0, self.dc0
            self.gemm_sk(self.dZ[:B], Ur, dh0, B, U, 4 * U, 4 * U, 4 * U, U, transB=True)
            self.gemm_sk(self.dqpre[0], a.p("attention/W2/kernel"), dh0, B, U, A, A, A, U, transB=True, accumulate=True)
        else:
            dh0, dc0 = self.dh_att, self.dc
            self.gemm_sk(self.dZ[:B], Ur, dh0, B, U, 4 * U, 4 * U, 4 * U, U, transB=True, accumulate=True)
        names = [f"{nm}/{w}" for nm in LearnedInitState.LAYERS for w in ("kernel", "bias")]
        grads = [None] * 4 if self._skip_grad(*names) else [a.g(n) for n in names]
        be.init_state_bwd(dh0, dc0, self.Hs[0], self.Cs[0], self.fmean, a.p("hidden_init/kernel"), a.p("carry_init/kernel"),
                          *grads, self.dF, B, R, D, U)

    def _coverage_launch(self, B, T, want_grad):
        """tnt_attention_coverage_f32 on the finished attention weights of the step: ``coverage`` into met[4], and with
        ``want_grad`` the gradient rider of the backward chain into cov_ext; a model without the term launches nothing"""
        cov = self.attention_coverage
        if cov is None:
            return
        self.be.attention_coverage(self.alpha, T, B, self.R, cov.axis_id, cov.coef(T, B, self.R) if want_grad else 0.0,
                                   self.cov_ext if want_grad else None, self.met[4:5], self.cov_work)

    def _coverage_key(self):
        cov = self.attention_coverage
        return cov.key if cov is not None else ()

    def _naive_check(self):
        """the shape the free-running decoder's feedback kernel is built for"""
        if self.Et % 4:
            raise NotImplementedError("the free-running decoder needs embedding_text % 4 == 0 (tnt_greedy_feedback_f32)")

    def _ss_check(self):
        """the descriptor and the shape scheduled sampling's feedback kernel is built for"""
        ss = self.scheduled_sampling
        if not isinstance(ss, ScheduledSampling):
            raise ValueError(f"scheduled_sampling must be None or a model_base.ScheduledSampling, got {ss!r}")
        if self.Et % 4 or self.Et > 1016:
            raise ValueError(f"scheduled sampling needs embedding_text % 4 == 0 and <= 1016 (tnt_scheduled_feedback2_f32), "
                             f"got {self.Et}")

    def _forward_ss(self, B, T):
        """The scheduled-sampling training forward (definition: include/tnt_hip.h, tnt_scheduled_feedback2_f32).  The
        teacher-forced front -- encoder, the Embedding of all T caption columns through the text Dropout and the LSTM
        input mask, XZ of step 0's rows -- then per step t the attention -> LSTM step, the teacher-forced LSTM-output
        Dropout on the step's rows, dense_inter, the output Dropout (logical (B, T, H): lwidth T*H, lcol0 t*H), dense_out
        into the step's logits rows and, for t + 1 < T, the feedback launch: it decides token position t + 1 of every row,
        writes a fed token into ``cap``, its doubly masked Embedding row into ``text`` and its projection into ``XZ``.
        The loss, its targets and the whole backward are the teacher-forced ones, over the fed ids.  At p = 1 this is not
        call_naive_attention: that mode's Dropouts differ (text Dropout on step 0 only, the output Dropout on the U-wide
        LSTM output, a second feature Dropout)."""
        be, a, ss = self.be, self.arena, self.scheduled_sampling
        D, U, Et, V, H, ldV = self.D, self.U, self.Et, self.V, self.H, self.ldV
        sd, ds = self.seed, self.drop_step
        self._encode(B, True)
        self._text_front(B, T, True, "ss")
        emb, Wl = a.p("emb_text/embeddings"), a.p("lstm/kernel")
        for t in range(T):
            rows = slice(t * B, (t + 1) * B)
            self._decode_step(t, B, True, xz_bias=a.p("lstm/bias"))
            h = self.Hs[t + 1]
            if self.r_lstm > 0:                                     # :256, site S_LSTM_OUT + t on the step's B rows
                be.dropout(h, self.Hd[rows], B, U, U, 0, U, 0, self.r_lstm, sd, S_LSTM_OUT + t, 0, ds)
                h = self.Hd[rows]
            self._head_inter(h, self.inter[rows], B, self.ipre[rows])
            inter = self.inter[rows]
            if self.r_out > 0:                                      # element (b*T + t)*H + j of the logical (B, T, H)
                be.dropout(inter, self.inter_d[rows], B, H, H, 0, T * H, t * H, self.r_out, sd, S_OUT, 0, ds)
                inter = self.inter_d[rows]
            self._head_out(inter, self.logits[rows], B)
            if t + 1 < T:
                col, nxt = t + 1, slice((t + 1) * B, (t + 2) * B)
                be.scheduled_feedback2(self.logits[rows], ldV, V, emb, Et, Wl[D:], 4 * U, 4 * U, self.cap, T, col,
                                       self.text[nxt], Et, self.XZ[nxt], 4 * U, B, self.r_lstm, sd, S_LSTM_IN + col, 0, ds,
                                       D + Et, D, ss.kind_id, ss.mode_id, self.ss_sched, self.adam_t, S_SS_COIN + t,
                                       S_SS_DRAW + t, self.r_text, S_TEXT, T * Et, col * Et)
        self._route.hs_used = self.Hd if self.r_lstm > 0 else self.Hs[1:].view(T * B, U)
        self._route.inter_used = self.inter_d if self.r_out > 0 else self.inter
        self._tail.metric_parts_ready = False      # the attention metric: _loss_metrics, behind the loop

    def _forward_naive(self, B, T, training):
        """lc_NIC.call_naive_attention (lc_NIC.py:175-221): the decoder fed its own greedy predictions.  Per step: attention
        -> LSTM step (per-step kernels: the head sits inside the recurrence, so the persistent chain cannot run) -> the
        LSTM-output and output Dropouts on the U-wide state in one pass -> dense_inter -> dense_out -> the feedback launch
        (tnt_greedy_feedback_f32: argmax -> fed id, its Embedding row through the next step's LSTM input mask, the text half
        of the next step's input projection).  The fed ids go to column i + 1 of ``self.cap`` in place: column 0 keeps
        the staged start token, and the backward pass scatters the Embedding gradient to exactly these ids."""
        be, a = self.be, self.arena
        D, U, Et, V, ldV = self.D, self.U, self.Et, self.V, self.ldV
        sd, ds = self.seed, self.drop_step
        self._encode(B, training, feat2=True)                                               # :180-184
        # step 0's input: the start token through the Embedding, the text Dropout (:187-189) and step 0's LSTM input mask,
        # as the teacher-forced step forms it (one launch over all T caption columns; rows 1.. are replaced by the fed ones)
        self._text_front(B, T, training, "naive")
        emb, Wl = a.p("emb_text/embeddings"), a.p("lstm/kernel")
        lstm_in = training and self.r_lstm > 0
        r_lo, r_o = (self.r_lstm, self.r_out) if training else (0.0, 0.0)
        for i in range(T):                                                                  # :191-219
            rows = slice(i * B, (i + 1) * B)
            self._decode_step(i, B, training, xz_bias=a.p("lstm/bias"))
            h = self.Hs[i + 1]
            if r_lo > 0 and r_o > 0:        # seq = dropout_lstm(a); output = dropout_output(seq)  (:205-207)
                be.dropout2(h, self.Hd[rows], B, U, U, (0, U, 0, 0, r_lo, S_LSTM_OUT + i), (0, U, 0, 0, r_o, S_NOUT + i), sd, 0, ds)
            elif r_lo > 0 or r_o > 0:
                be.dropout(h, self.Hd[rows], B, U, U, 0, U, 0, max(r_lo, r_o), sd, S_LSTM_OUT + i if r_lo > 0 else S_NOUT + i, 0, ds)
            if r_lo > 0 or r_o > 0:
                h = self.Hd[rows]
            self._head_inter(h, self.inter[rows], B, self.ipre[rows])                       # :209
            self._head_out(self.inter[rows], self.logits[rows], B)                          # :211
            if i + 1 < T:                                                                   # :215-217
                nxt = slice((i + 1) * B, (i + 2) * B)
                be.greedy_feedback(self.logits[rows], ldV, V, emb, Et, Wl[D:], 4 * U, 4 * U, self.cap, T, i + 1, self.text[nxt],
                                   Et, self.XZ[nxt], 4 * U, B, self.r_lstm if lstm_in else 0.0, sd, S_LSTM_IN + i + 1, 0, ds,
                                   lwidth=D + Et, lcol0=D)
        self._route.hs_used = self.Hd if (r_lo > 0 or r_o > 0) else self.Hs[1:].view(T * B, U)
        self._route.inter_used = self.inter
        self._tail.metric_parts_ready = False

    def _loss_metrics(self, B, T, want_grad):
        be = self.be
        n = T * B
        self._head_loss(B, T, want_grad)
        self._sum2(self.loss_row, self.met[0:1], self.corr_row, self.met[1:2], n, 1.0 / n)
        if self.S == 1:
            npart = be.attention_metric_parts(T, self.R)
            t = self._tail
            if t.deferring and want_grad and 0 < npart <= self.metric_part.numel():
                # fused single-process step: partials only, their total rides in the step-finalize launch
                if not t.metric_parts_ready:
                    be.attention_metric(self.alpha, None, self.metric_part, T, B, self.R)
                t.x2, t.out2, t.n2, t.scale2 = self.metric_part, self.met[3:4], npart, 1.0 / (T * self.R)
            else:
                be.attention_metric(self.alpha, self.met[3:4], self.metric_part, T, B, self.R)              # :365-367
        else:       # per-subject loss / accuracy / attention metric (ms2_NIC.py:324-372)
            S, Bs = self.S, B // self.S
            be.colsum(self.loss_row, self.colB[:B], T, B, B, self.work)
            be.colsum(self.corr_row, self.colB[B:], T, B, B, self.work)
            for q in range(S):
                k = 8 + 4 * q
                be.sum(self.colB[q * Bs:], self.met[k:k + 1], Bs, 1.0 / (Bs * T))
                be.sum(self.colB[B + q * Bs:], self.met[k + 1:k + 2], Bs, 1.0 / (Bs * T))
                be.attention_metric(self.alpha.view(-1)[q * Bs * self.R:], self.met[k + 2:k + 3], self.metric_part, T, Bs,
                                    self.R, B * self.R)
        if want_grad and self._distill_on():
            self._distill_metric(n)     # the finalize launch's third slot is the attention metric's: a launch of its own then

    # ------------------------------------------------------------------ backward
    def _backward(self, B, T):
        """tape.gradient (lc_NIC.py:386-387) as four launch groups, in the order the gradients become final -- the
        data-parallel schedule (dp.PipelinedAttentionSync) issues one all-reduce bucket after each."""
        self._bwd_head(B, T)
        self._bwd_chain(B, T)
        self._bwd_init(B, T)
        # the text branch (input Dropout', sparse Embedding scatter) and the front branch (attention parameters, BatchNorm,
        # region-wise encoder) only share the chain's outputs: with `branch_streams` they are two parallel branches of the step
        with self.side(0 if self.branch_streams else -1):
            self._bwd_emb(B, T)
        self._bwd_front(B, T)
        self.join()

    def _bwd_head(self, B, T):
        """vocabulary head: gradients of time_distributed_softmax / time_distributed_nonlinear, dHs.  The free-running
        step (teacher_forcing=False) has no Dropout between dense_inter and dense_out: its fused tail runs at rate 0, and the LSTM-output and the output Dropout' both act on dHs (lc_NIC.py:205-211)."""
        be, a = self.be, self.arena
        U, V, H, ldV = self.U, self.V, self.H, self.ldV
        n = T * B
        sd, ds = self.seed, self.drop_step
        naive = not self.teacher_forcing
        route = self._route
        dlog, inter, hs = self.logits, route.inter_used, route.hs_used         # (free-running: inter_used is self.inter)
        tB, r_tail = (0, 0.0) if naive else (B, self.r_out)
        dhs_done = False
        head_frozen = self._skip_grad("time_distributed_softmax/kernel", "time_distributed_softmax/bias")
        if head_frozen:
            # a frozen softmax layer: its input gradient alone.  (Its bias gradient's column sums share the launch below
            # with the nonlinear layer's Dropout' / LeakyReLU' / bias gradient, which is still needed: that launch stays)
            self.gemm_sk(dlog, a.p("time_distributed_softmax/kernel"), self.dinter, n, H, V, ldV, ldV, H, transB=True)
        # kernel gradient and input gradient of the softmax layer, the two independent readers of dlogits: ONE launch
        elif not (self.g3_riders and self.gemm3_pair(
                dict(A=inter, B=dlog, C=a.g("time_distributed_softmax/kernel"), M=H, N=V, K=n, lda=H, ldb=ldV, ldc=ldV, transA=True),
                dict(A=dlog, B=a.p("time_distributed_softmax/kernel"), C=self.dinter, M=n, N=H, K=V, lda=ldV, ldb=ldV, ldc=H,
                     transB=True))):
            self.gemm_sk(inter, dlog, a.g("time_distributed_softmax/kernel"), H, V, n, H, ldV, ldV, transA=True)
            self.gemm_sk(dlog, a.p("time_distributed_softmax/kernel"), self.dinter, n, H, V, ldV, ldV, H, transB=True)
        if n <= 2048 and H % 4 == 0:
            # dropout' + LeakyReLU' + the nonlinear layer's bias gradient in one pass over dinter, with the softmax layer's
            # bias gradient (column sums of dlogits) riding in the same launch: 1 launch instead of 4
            be.bias_act_drop_bwd(self.dinter, self.ipre, self.dinter, a.g("time_distributed_nonlinear/bias"), n, H, H,
                                 ACT_LEAKY, 0.2, tB, H, 0, r_tail, sd, S_OUT, ds,
                                 extra=(dlog, a.g("time_distributed_softmax/bias"), n, V, ldV))
            # kernel gradient and input gradient of the nonlinear layer, the two readers of dinter: ONE launch
            if self.g3_riders and self.gemm3_pair(
                    dict(A=hs, B=self.dinter, C=a.g("time_distributed_nonlinear/kernel"), M=U, N=H, K=n, lda=U, ldb=H, ldc=H,
                         transA=True, small=True),
                    dict(A=self.dinter, B=a.p("time_distributed_nonlinear/kernel"), C=self.dHs, M=n, N=U, K=H, lda=H, ldb=H, ldc=U,
                         transB=True, small=True)):
                dhs_done = True
            else:
                self.gemm_sk(hs, self.dinter, a.g("time_distributed_nonlinear/kernel"), U, H, n, U, H, H, transA=True)
        else:
            if not head_frozen:         # (a launch of its own here: a frozen softmax layer has none)
                be.colsum(dlog, a.g("time_distributed_softmax/bias"), n, V, ldV, self.work)
            if r_tail > 0:
                be.dropout(self.dinter, self.dinter, n, H, H, B, H, 0, r_tail, sd, S_OUT, 0, ds)
            be.act_bwd(self.ipre, self.dinter, self.dinter, n * H, ACT_LEAKY, 0.2)
            self.gemm_sk(hs, self.dinter, a.g("time_distributed_nonlinear/kernel"), U, H, n, U, H, H, transA=True)
            be.colsum(self.dinter, a.g("time_distributed_nonlinear/bias"), n, H, H, self.work)
        if not dhs_done:
            self.gemm_sk(self.dinter, a.p("time_distributed_nonlinear/kernel"), self.dHs, n, U, H, H, H, U, transB=True)
        r_lo, r_o = self.r_lstm, self.r_out
        if not naive:
            route.dout_masked = not (r_lo > 0 and self._lc_seq_bwd_ok())
            if r_lo > 0 and route.dout_masked:              # (else Dropout' rides in the backward chain: tnt_lc_seq_bwd_drop_f32)
                be.dropout(self.dHs, self.dHs, n, U, U, 0, U, 0, r_lo, sd, S_LSTM_OUT, 0, ds, rows_per_site=B)
            return
        route.dout_masked = True            # both masks are applied here, none rides in the backward chain
        if r_lo > 0 and r_o > 0:
            be.dropout2(self.dHs, self.dHs, n, U, U, (0, U, 0, B, r_lo, S_LSTM_OUT), (0, U, 0, B, r_o, S_NOUT), sd, 0, ds)
        elif r_lo > 0 or r_o > 0:
            be.dropout(self.dHs, self.dHs, n, U, U, 0, U, 0, max(r_lo, r_o), sd, S_LSTM_OUT if r_lo > 0 else S_NOUT, 0, ds,
                       rows_per_site=B)

    def _lc_seq_bwd_ok(self):
        """the persistent backward-chain kernel applies (tnt_lc_seq_bwd_f32: the forward chain's shape limits)."""
        return bool(not self.use_layer_norm and self._lc_seq_ok() and self.lc_xch is not None and self.use_lc_seq_bwd)

    def _bwd_chain(self, B, T):
        """the T-step chain (LSTM step backward -> attention step backward) and the LSTM parameter gradients."""
        be, a = self.be, self.arena
        R, D, A, U, Et = self.R, self.D, self.A, self.U, self.Et
        n = T * B
        sd, ds = self.seed, self.drop_step
        # no zero fill of dP / dF / dvb: the first executed step (i = T-1) overwrites them (fresh)
        Wl, Ur = a.p("lstm/kernel"), a.p("lstm/recurrent_kernel")
        W2, v = a.p("attention/W2/kernel"), a.p("attention/V/kernel")
        route = self._route
        route.dtext_done = route.dw2_done = False
        if self.use_layer_norm:
            return self._bwd_chain_ln(B, T)
        if self._lc_seq_bwd_ok():
            # the T LSTM-backward -> attention-backward steps as ONE persistent launch (tnt_lc_seq_bwd_f32): role-specialised
            # workgroups per XCD, dP / dF / dvb accumulated on chip and written once
            keep = self.att_keep if self._keep_stored else None
            be.lc_seq_bwd(self.F, self.P, W2, v, self.qpre, self.alpha, keep, B * R * A // 4 if keep is not None else 0,
                          self.dP, self.dF, self.dvb, self.dqpre, Ur, Wl[:D], self.dHs, self.gates, self.Cs, self.dZ,
                          self.lc_xch, T, B, R, D, A, U, 0.2, self.r_attn, self.r_lstm, D + Et, sd, S_ATTN, S_LSTM_IN, ds,
                          self._alpha_mse, self.seq_sync, self._guard_out(),
                          out_drop=None if route.dout_masked else (self.r_lstm, S_LSTM_OUT),
                          **({} if self.attention_coverage is None
                             else dict(ext=(self.cov_ext,) + self.attention_coverage.strides(R))),
                          **({} if self.init_state is None else dict(dc0=self.dc0)))
        else:
            self._bwd_chain_steps(B, T, Wl, Ur, W2, v)
        hprev = self.Hs[:T].view(n, U)
        gWl = a.g("lstm/kernel")
        if self._skip_grad("lstm/kernel", "lstm/recurrent_kernel", "lstm/bias"):
            # a frozen LSTM: none of its parameter gradients; _bwd_emb forms dtext and _bwd_front the W2 gradient alone
            return
        if self.g3_riders and Et == U and self.gemm3_pair(
                dict(A=hprev, B=self.dZ, C=a.g("lstm/recurrent_kernel"), M=U, N=4 * U, K=n, lda=U, ldb=4 * U, ldc=4 * U, transA=True,
                     colsum=a.g("lstm/bias"), A2=self.text, C2=gWl[D:]),
                dict(A=self.dZ, B=Wl[D:], C=self.dtext, M=n, N=Et, K=4 * U, lda=4 * U, ldb=4 * U, ldc=Et, transB=True)):
            # the four readers of dZ that fill the chip -- recurrent-kernel gradient, the text rows of the kernel gradient (+ the
            # bias gradient as a rider) and the text-input gradient (_bwd_emb finds it done) -- in ONE launch
            route.dtext_done = True
            # ... and the two small kernel gradients that only need the chain's outputs -- the context rows of the LSTM kernel
            # and the attention's W2 -- in one launch behind it
            route.dw2_done = bool(self.gemm3_pair(
                dict(A=self.ctx_d, B=self.dZ, C=gWl[:D], M=D, N=4 * U, K=n, lda=D, ldb=4 * U, ldc=4 * U, transA=True, small=True),
                dict(A=hprev, B=self.dqpre, C=a.g("attention/W2/kernel"), M=U, N=A, K=n, lda=U, ldb=A, ldc=A, transA=True,
                     small=True)))
            if not route.dw2_done:
                self.gemm_sk(self.ctx_d, self.dZ, gWl[:D], D, 4 * U, n, D, 4 * U, 4 * U, transA=True)
            return
        if self.g3_riders and Et == U and self.gemm3(
                hprev, self.dZ, a.g("lstm/recurrent_kernel"), U, 4 * U, n, U, 4 * U, 4 * U, transA=True,
                colsum=a.g("lstm/bias"), A2=self.text, C2=gWl[D:]):
            # recurrent-kernel gradient, the text rows of the kernel gradient and the bias gradient in ONE launch: the two
            # products share dZ, its column sums ride on the fragments the first tile row holds anyway
            self.gemm_sk(self.ctx_d, self.dZ, gWl[:D], D, 4 * U, n, D, 4 * U, 4 * U, transA=True)
            return
        self.gemm_sk(hprev, self.dZ, a.g("lstm/recurrent_kernel"), U, 4 * U, n, U, 4 * U, 4 * U, transA=True)
        self.gemm_sk(self.text, self.dZ, gWl[D:], Et, 4 * U, n, Et, 4 * U, 4 * U, transA=True)
        self.gemm_sk(self.ctx_d, self.dZ, gWl[:D], D, 4 * U, n, D, 4 * U, 4 * U, transA=True)
        be.colsum(self.dZ, a.g("lstm/bias"), n, 4 * U, 4 * U, self.work)

    def _bwd_chain_steps(self, B, T, Wl, Ur, W2, v):
        """the chain as 2 T per-step launches"""
        be = self.be
        R, D, A, U, Et = self.R, self.D, self.A, self.U, self.Et
        sd, ds = self.seed, self.drop_step
        cov = self.attention_coverage
        ext_ts, ext_bs = cov.strides(R) if cov is not None else (0, 0)
        for i in range(T - 1, -1, -1):
            last = i == T - 1
            # the coverage gradient of this step's attention weights: its slab of the rider (every step's for axis="time")
            ext = {} if cov is None else dict(ext=self.cov_ext[i * ext_ts:], ext_bs=ext_bs)
            # dctx_i = dZ_i @ Wc^T: every LSTM-backward workgroup leaves the partial of its 16 units, the attention
            # backward sums the U/16 parts (instead of running the whole product per sample on its own critical path)
            parts = (U // 16) * D <= 1024
            be.lstm_step_bwd(None if last else self.dZ[(i + 1) * B:(i + 2) * B], Ur, None,
                             None if last else self.dh_att, None if last else self.dc, None,
                             self.dHs[i * B:(i + 1) * B], None, 0, 0, self.gates[i], self.Cs[i + 1], self.Cs[i],
                             self.dZ[i * B:(i + 1) * B], None, self.dc, None, B, U,
                             Wc=Wl[:D] if parts else None, D=D, dctx_part=self.dctx_part if parts else None)
            if parts:
                be.attention_step_bwd(None, self.F, self.P, W2, v, self.qpre[i], self.alpha[i], self.dP, self.dF,
                                      self.dvb, self.dqpre[i], self.dh_att, B, R, D, A, U, 0.2, self.r_attn, self.r_lstm,
                                      D + Et, sd, S_ATTN + i, S_LSTM_IN + i, 0, ds, dctx_part=self.dctx_part,
                                      nparts=U // 16, keep4=self.att_keep[i] if self._keep_stored else None,
                                      alpha_mse=self._alpha_mse, fresh=last, **ext)
            else:
                be.attention_step_bwd(None, self.F, self.P, W2, v, self.qpre[i], self.alpha[i], self.dP, self.dF,
                                      self.dvb, self.dqpre[i], self.dh_att, B, R, D, A, U, 0.2, self.r_attn, self.r_lstm,
                                      D + Et, sd, S_ATTN + i, S_LSTM_IN + i, 0, ds, dz=self.dZ[i * B:(i + 1) * B],
                                      Wc=Wl[:D], keep4=self.att_keep[i] if self._keep_stored else None,
                                      alpha_mse=self._alpha_mse, fresh=last, **ext)

    def _bwd_chain_ln(self, B, T):
        """The T-step chain with the LayerNormLSTMCell (reverse of _decode_step's LayerNorm branch).  Per step: cell
        backward (gate math + state LayerNorm) -> input gradients of the two 4U-wide LayerNorms -> dh of the previous
        step through U^T -> attention step backward (context gradient from dZK).  The parameter gradients of the three
        LayerNorms and of W / U / b are batched over all T steps behind the chain."""
        be, a = self.be, self.arena
        R, D, A, U, Et = self.R, self.D, self.A, self.U, self.Et
        n = T * B
        sd, ds = self.seed, self.drop_step
        Wl, Ur = a.p("lstm/kernel"), a.p("lstm/recurrent_kernel")
        W2, v = a.p("attention/W2/kernel"), a.p("attention/V/kernel")
        gk, gr, gs = a.p("lstm/kernel_norm/gamma"), a.p("lstm/recurrent_norm/gamma"), a.p("lstm/state_norm/gamma")
        for i in range(T - 1, -1, -1):
            last = i == T - 1
            rows = slice(i * B, (i + 1) * B)
            be.ln_lstm_cell_bwd(self.dHs[rows], None if last else self.dh_att, None if last else self.dh_rec,
                                None if last else self.dc, self.gates[i], self.Cs[i], self.Cs[i + 1], self.chat[rows],
                                self.is_s[i], gs, self.dZ[rows], self.dc, self.dcnt[rows], B, U)
            be.layernorm_bwd(self.dZ[rows], self.xh_k[rows], gk, self.is_k[i], self.dZK[rows], None, None, B, 4 * U, 4 * U, None)
            be.layernorm_bwd(self.dZ[rows], self.xh_r[rows], gr, self.is_r[i], self.dZR[rows], None, None, B, 4 * U, 4 * U, None)
            self.gemm_sk(self.dZR[rows], Ur, self.dh_rec, B, U, 4 * U, 4 * U, 4 * U, U, transB=True)
            be.attention_step_bwd(None, self.F, self.P, W2, v, self.qpre[i], self.alpha[i], self.dP, self.dF,
                                  self.dvb, self.dqpre[i], self.dh_att, B, R, D, A, U, 0.2, self.r_attn, 0.0,
                                  D + Et, sd, S_ATTN + i, S_LSTM_IN + i, 0, ds, dz=self.dZK[rows],
                                  Wc=Wl[:D], keep4=self.att_keep[i] if self._keep_stored else None,
                                  alpha_mse=self._alpha_mse, fresh=last)
        hprev = self.Hs[:T].view(n, U)
        gWl = a.g("lstm/kernel")
        self.gemm_sk(hprev, self.dZR, a.g("lstm/recurrent_kernel"), U, 4 * U, n, U, 4 * U, 4 * U, transA=True)
        self.gemm_sk(self.text, self.dZK, gWl[D:], Et, 4 * U, n, Et, 4 * U, 4 * U, transA=True)
        self.gemm_sk(self.ctx_d, self.dZK, gWl[:D], D, 4 * U, n, D, 4 * U, 4 * U, transA=True)
        # gamma / beta of the three LayerNorms, summed over all T*B rows: dgamma = sum dy * xhat, dbeta = sum dy
        be.layernorm_bwd(self.dZ, self.xh_k, gk, self.is_k, None, a.g("lstm/kernel_norm/gamma"), a.g("lstm/kernel_norm/beta"),
                         n, 4 * U, 4 * U, self.work)
        be.layernorm_bwd(self.dZ, self.xh_r, gr, self.is_r, None, a.g("lstm/recurrent_norm/gamma"),
                         a.g("lstm/recurrent_norm/beta"), n, 4 * U, 4 * U, self.work)
        be.layernorm_bwd(self.dcnt, self.chat, gs, self.is_s, None, a.g("lstm/state_norm/gamma"), a.g("lstm/state_norm/beta"),
                         n, U, U, self.work)
        be.colsum(self.dZ, a.g("lstm/bias"), n, 4 * U, 4 * U, self.work)

    def _bwd_emb(self, B, T):
        """text branch: dtext = dZ Wl_text^T, its dropouts, the embedding scatter (+ IndexedSlices norm).  Free-running
        (teacher_forcing=False): the LSTM input mask' on every step's text rows, the text Dropout' on step 0's only (the
        fed tokens have none, lc_NIC.py:217), the scatter to the fed ids."""
        be, a = self.be, self.arena
        if self._skip_grad("emb_text/embeddings"):
            # a frozen Embedding: dtext feeds nothing else, so neither its product nor its Dropout' nor the scatter run (where
            # the chain's pair launch formed dtext beside the LSTM gradients, that launch stays)
            return
        D, U, Et, V = self.D, self.U, self.Et, self.V
        n = T * B
        sd, ds = self.seed, self.drop_step
        naive = not self.teacher_forcing
        Wl = a.p("lstm/kernel")
        if not self._route.dtext_done:
            self.gemm_sk(self.dZK if self.use_layer_norm else self.dZ, Wl[D:], self.dtext, n, Et, 4 * U, 4 * U, 4 * U, Et, transB=True)
        lstm_in = self.r_lstm > 0 and not self.use_layer_norm
        if not naive and lstm_in and self.r_text > 0 and Et % 4 == 0 and D % 4 == 0:
            # the LSTM input mask and the Embedding Dropout of the text rows in one pass
            be.dropout2(self.dtext, self.dtext, n, Et, Et, (0, D + Et, D, B, self.r_lstm, S_LSTM_IN),
                        (B, Et, 0, 0, self.r_text, S_TEXT), sd, 0, ds)
        else:
            if lstm_in:
                be.dropout(self.dtext, self.dtext, n, Et, Et, 0, D + Et, D, self.r_lstm, sd, S_LSTM_IN, 0, ds,
                           rows_per_site=B)
            if self.r_text > 0 and naive:      # step 0's rows of the logical (B, T, Et) mask the forward's Embedding launch applied
                be.dropout(self.dtext[:B], self.dtext[:B], B, Et, Et, 0, T * Et, 0, self.r_text, sd, S_TEXT, 0, ds)
            elif self.r_text > 0:
                be.dropout(self.dtext, self.dtext, n, Et, Et, B, Et, 0, self.r_text, sd, S_TEXT, 0, ds)
        self._route.emb_rows = (self.dtext, n, Et, Et, "emb_text/embeddings")
        self._embedding_bwd(self.dtext, self.cap, "emb_text/embeddings", B, T, Et, Et, V)

    def _bwd_front(self, B, T):
        """attention parameters, then BatchNorm / region-wise encoder backward."""
        be, a = self.be, self.arena
        R, D, A, U = self.R, self.D, self.A, self.U
        n = T * B
        sd, ds = self.seed, self.drop_step
        hprev = self.Hs[:T].view(n, U)
        # attention parameters
        if not self._route.dw2_done:
            self.gemm_sk(hprev, self.dqpre, a.g("attention/W2/kernel"), U, A, n, U, A, A, transA=True)
        jobs = [(self.dqpre, a.g("attention/W2/bias"), n, A, A), (self.dvb, a.g("attention/V/kernel"), B, A, A + 1),
                (self.dvb.view(-1)[A:], a.g("attention/V/bias"), B, 1, A + 1)]
        if n <= 2048 and B <= 2048:
            be.colsum_multi(jobs)                     # the three small bias-type gradients of the attention layer: one launch
        else:
            for x, out, rows, C, ld in jobs:
                be.colsum(x, out, rows, C, ld, self.work)
        fdrop = None                                   # (rate, seed, site, step_dev) of the Dropout' folded into the dF pass
        if D == 32 and A == 32:
            # LeakyReLU' + bias gradient + W1 gradient + the dF contribution of the hoisted Dense in two launches instead of five
            fb = self._att_fb
            if fb is None or fb[1] != (B * R, D, A):
                if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("attention front-backward scratch must be built outside a graph capture")
                fb = self._att_fb = (self._f(be.attention_front_bwd_parts(B * R, D, A)), (B * R, D, A))
            # dF is finished by this launch: the backward of the LAST feature Dropout (one site over all B*R rows: the
            # deepest stage's, or the single-subject encoder's) rides in its dF pass
            if self.r_feat > 0 and self.fused_bn_drop and (self.depth > 0 or self.S == 1):
                fdrop = (self.r_feat, sd, S_DEEP + self.depth - 1 if self.depth > 0 else S_FEAT, ds)
            be.attention_front_bwd(self.Ppre, self.dP, self.F, a.p("attention/W1/kernel"), self.dF,
                                   a.g("attention/W1/kernel"), a.g("attention/W1/bias"), fb[0], B * R, D, A, 0.2, drop=fdrop)
        else:
            be.act_bwd(self.Ppre, self.dP, self.dP, B * R * A, ACT_LEAKY, 0.2)
            self.gemm_sk(self.F, self.dP, a.g("attention/W1/kernel"), D, A, B * R, D, A, A, transA=True)
            be.colsum(self.dP, a.g("attention/W1/bias"), B * R, A, A, self.work)
            self.gemm_sk(self.dP, a.p("attention/W1/kernel"), self.dF, B * R, D, A, A, A, D, transB=True, accumulate=True)
        if not self.teacher_forcing and self.r_feat > 0:     # the second feature Dropout of call_naive_attention (:184)
            be.dropout(self.dF, self.dF, B * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT2, 0, ds)
        # encoder
        S = self.S
        Bs = B // S
        dF_enc = self.dF
        for i in range(self.depth - 1, -1, -1):          # the deep stages, last first; dF_enc: gradient wrt Fs[i + 1]
            bn = f"input_bn/deep{i}"
            if self.r_feat > 0 and not (fdrop is not None and i == self.depth - 1):
                be.dropout(dF_enc, dF_enc, B * R, D, D, 0, D, 0, self.r_feat, sd, S_DEEP + i, 0, ds)
            acted = False
            if self.norm == "batch":
                acted = self._bn_bwd(dF_enc, self.deep_xhat[i], a.p(f"{bn}/gamma"), self.deep_istd[i], self.dbn,
                                     a.g(f"{bn}/gamma"), a.g(f"{bn}/beta"), B * R, D, D, self.work, act_pre=self.deep_pre[i])
            else:
                be.layernorm_bwd(dF_enc, self.deep_xhat[i], a.p(f"{bn}/gamma"), self.deep_istd[i], self.dbn,
                                 a.g(f"{bn}/gamma"), a.g(f"{bn}/beta"), B * R, D, D, self.work)
            if not acted:
                be.act_bwd(self.deep_pre[i], self.dbn, self.dbn, B * R * D, ACT_LEAKY, 0.2)
            be.locally_dense_bwd(self.Fs[i], R * D, self.deep_idx, self.deep_goff, self.dbn, self.deepWg[i], self.deepBg[i],
                                 B, R, D)
            be.block_dense_dx(self.dbn, self.deepW[i], self.dFd, B, R, D, D)
            dF_enc = self.dFd
        for q in range(S):
            off = SUBJ_SITE * (q + 1) if S > 1 else 0
            r0, r1 = q * Bs, (q + 1) * Bs
            dFq, xh, dbn = dF_enc[r0:r1], self.xhat[r0 * R:r1 * R], self.dbn[r0 * R:r1 * R]
            if self.r_feat > 0:
                if S > 1:
                    be.dropout(dFq, dFq, Bs * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT2 + off, 0, ds)
                if not (fdrop is not None and self.depth == 0):
                    be.dropout(dFq, dFq, Bs * R, D, D, 0, D, 0, self.r_feat, sd, S_FEAT + off, 0, ds)
            bn = self.bn_name(q)
            acted = False
            if self.norm == "batch":
                acted = self._bn_bwd(dFq, xh, a.p(f"{bn}/gamma"), self.inv_std[q], dbn, a.g(f"{bn}/gamma"),
                                     a.g(f"{bn}/beta"), Bs * R, D, D, self.work, act_pre=self.enc_pre[r0:r1])
            else:
                be.layernorm_bwd(dFq, xh, a.p(f"{bn}/gamma"), self.inv_std[q], dbn, a.g(f"{bn}/gamma"),
                                 a.g(f"{bn}/beta"), Bs * R, D, D, self.work)
            if not acted:
                be.act_bwd(self.enc_pre[r0:r1], dbn, dbn, Bs * R * D, ACT_LEAKY, 0.2)
            x = (self.xd if self.r_in > 0 else self.x)[r0:r1]
            if self.NV > R and hasattr(be, "locally_dense_bwd_split") and self.split_encoder:
                vm = self.xT is not None and self.voxel_major
                be.locally_dense_bwd_split(self.xT[:, r0:r1] if vm else x, self.xT.shape[1] if vm else self.ldx, self.idx,
                                           self.vgoff, self.vreg, self.vfirst, self.NV, dbn, self.encWg[q], self.encBg[q],
                                           Bs, R, D, voxel_major=vm)
            else:
                be.locally_dense_bwd(x, self.ldx, self.idx, self.goff, dbn, self.encWg[q], self.encBg[q], Bs, R, D)

    # ------------------------------------------------------------------ steps
    def _train_graph(self, B, T):
        if self.scheduled_sampling is not None:
            self._forward_ss(B, T)
        else:
            (self._forward if self.teacher_forcing else self._forward_naive)(B, T, True)
        self._loss_metrics(B, T, True)
        self._coverage_launch(B, T, True)          # behind the forward chain, in front of the backward chain that reads it
        self._backward(B, T)

    def _stage_mask_job(self):
        if not self._keep_stored:
            return None
        B, T = self._shape
        return (self.att_keep, B * self.R * self.A, T, self.r_attn, self.seed, S_ATTN, self.drop_step)

    def _metrics(self, with_lr, ring=False, distill=False):
        m = self._met_snapshot(ring)
        if self.S == 1:
            out = Metrics(loss=m[0], L2=m[2], accuracy=m[1], attention=m[3])
            if self.attention_coverage is not None:
                out["coverage"] = m[4]              # unweighted; ``loss`` stays the cross-entropy
            if distill:
                out["distill_kl"] = m[self.DISTILL_KL]
        else:       # keys of ms2_NIC.train_step's return dict (ms2_NIC.py:366-374), A, B, C ... per subject
            out = Metrics(loss=m[0], L2=m[2])
            for q in range(self.S):
                tag, k = chr(ord("A") + q), 8 + 4 * q
                out[f"loss{tag}"], out[f"accuracy{tag}"], out[f"attention{tag}"] = m[k], m[k + 1], m[k + 2]
        if with_lr:
            if self.lr_schedule is not None:
                self._lr_metric(out)                                          # computed on the device: read from there
            else:
                out["lr"] = torch.tensor(self._lr_host, dtype=torch.float32)  # host-set (ModelBase._sync_lr): no device copy
        out._ring = self._last_ring
        return out.guarded(self, m[self.GUARD]) if self._seq_lstm else out

    def train_step(self, data):
        """lc_NIC.train_step (lc_NIC.py:328-408): returns {loss, L2, accuracy, attention, lr}."""
        if self.optimizer is None:
            raise RuntimeError("compile() the model before train_step")
        compat.check(self, self.STEP_FEATURES)       # (grad_sync may have been attached since the constructor)
        self._sync_accum()
        distill = self._distill_begin()
        B, T = self._stage_batch(data[0], data[1], self.n_in, masks=True, corrupt=True)
        self._ss_refuse(T)
        if distill:
            self._teach(data, B, T)
            self._distill_bufs(B, T)        # behind it: the teacher may just have rebuilt its buffers
        self._sync_lr()
        ring = False
        if self._accum_host is not None:    # gradient_accumulation_steps=k: ModelBase._train_step_accum
            if self._train_step_accum(B, T):
                self.optimizer.iterations += 1
            return self._metrics(True)
        if self.grad_sync is None:
            ring = self._run_step(self._step_runner(self.Et), ("train", B, T) + self._coverage_key() + (("distill",) if distill else ()),
                                  lambda: self._train_and_update_graph(B, T))
        elif getattr(self.grad_sync, "pipelined", False):
            self.grad_sync.step(self, B, T)
        else:
            self._train_step_dp(B, T, lambda: self._train_graph(B, T), self._update_graph)
        self.optimizer.iterations += 1
        return self._metrics(True, ring, distill)

    _alpha_mse = 0.0        # coefficient of the attention-MSE gradient in the backward chain (train_step_sam's first pass)

    def train_step_sam(self, data, rho=0.05):
        """lc_NIC.train_step_sam (lc_NIC.py:713-838): sharpness-aware step.  Pass 1 differentiates
        CE + L2 + MSE(ones, attention_scores) (:751-766), the weights move by e_w = g * rho / (global_norm(g) + 1e-12)
        (:768-786; the Embedding's IndexedSlices enter the norm by their un-deduplicated values), pass 2 differentiates
        CE + L2 there (:800-830), the weights are restored and the optimizer applies the second gradient (:833-836).
        Returns {loss, L2, accuracy, attention = MSE(ones, alpha), lr} of the second pass (:838).  Both passes draw the
        same dropout masks.  One captured launch sequence: two forward / backward passes and the update."""
        if self.optimizer is None:
            raise RuntimeError("compile() the model before train_step_sam")
        compat.check(self, ("sam", "corruption"), sam="train_step_sam")
        B, T = self._stage_batch(data[0], data[1], self.n_in, masks=True, corrupt=True)      # both passes read this batch
        self._sync_lr()
        be, a = self.be, self.arena
        if self.ew is None:
            self.ew = torch.zeros_like(a.theta)
        n_alpha = T * B * self.R

        def run():
            self._forward(B, T, True)
            self._loss_metrics(B, T, True)
            self._alpha_mse = 2.0 / n_alpha
            try:
                self._backward(B, T)
            finally:
                self._alpha_mse = 0.0
            self._norms_and_l2(None)
            self._sam_move(rho, 0, a.sq_override)
            self._forward(B, T, True)
            self._loss_metrics(B, T, True)
            be.sqdiff_mean(self.alpha, self.met[3:4], n_alpha, 1.0)
            self._backward(B, T)
            self._norms_and_l2(self.met[2:3])          # L2 as the reference reports it: at the perturbed weights
            self._sam_move(rho, 1)
            self._apply_agc()
            self._norms_and_l2(None)                   # clip norms of the second gradient at the restored weights
            self._apply_optimizer()
        self._run_captured(("sam", B, T, float(rho)), run)
        self.optimizer.iterations += 1
        return self._metrics(True)

    def test_step(self, data):
        """lc_NIC.test_step (lc_NIC.py:410-459)."""
        B, T = self._stage_batch(data[0], data[1], self.n_in)

        # ms2_NIC.test_step calls its sub-models with training=True (ms2_NIC.py:419,426) -- quirk kept
        train_flag = self.S > 1

        def run():
            (self._forward if self.teacher_forcing else self._forward_naive)(B, T, train_flag)
            self._loss_metrics(B, T, False)
            self._coverage_launch(B, T, False)      # the value only
            self._norms_and_l2(self.met[2:3])
            if train_flag:
                self.be.step_tick(None, self.drop_step, None, None, 0.0, 0.0)
        self._run_captured(("test", B, T) + self._coverage_key(), run)
        return self._metrics(False)

    def __call__(self, data, training=False):
        """lc_NIC.call -> call_attention (lc_NIC.py:163-164,223-263), or call_naive_attention with teacher_forcing=False:
        returns (probabilities (B,T,V), attention scores (T,B,R,1))."""
        if not self.teacher_forcing:
            return self.call_naive_attention(data, training)
        return self.call_attention(data, training)

    call = __call__

    def call_attention(self, data, training=False):
        """lc_NIC.call_attention (lc_NIC.py:223-263): returns (probabilities (B,T,V), attention scores (T,B,R,1))."""
        B, T = self._stage_inputs(data)

        def run():
            self._forward(B, T, training)
            return self._probs(B, T), self.alpha.clone().unsqueeze(-1)
        return self._guarded(run)

    def call_naive_attention(self, data, training=False, return_ids=False):
        """lc_NIC.call_naive_attention (lc_NIC.py:175-221): only the caption's start token (column 0) is read; every
        later step is fed the argmax of the step before.  Returns (probabilities (B,T,V), attention scores (T,B,R,1)),
        plus the predicted ids (B,T) int32 (the argmax of every step's output) with return_ids=True.  The argmax is taken
        over the logits (include/tnt_hip.h: tnt_greedy_feedback_f32)."""
        # the decoder of this call is the free-running one, whatever the model trains with
        compat.check(self, ("multi_subject", "layer_norm_lstm"), teacher_forcing=False)
        self._naive_check()
        B, T = self._stage_inputs(data)

        def run():
            self._forward_naive(B, T, training)
            self.be.argmax_rows(self.logits[(T - 1) * B:], self.last_ids, B, self.V, self.ldV)
            out = (self._probs(B, T), self.alpha.clone().unsqueeze(-1))
            if return_ids:
                out += (torch.cat([self.cap[:, 1:], self.last_ids.view(B, 1)], dim=1),)
            return out
        return self._guarded(run)

    def fed_ids(self):
        """(B, T) int32 numpy: the tokens the last free-running pass fed its decoder steps (column 0: the start token)"""
        return self.cap.cpu().numpy().copy()

    def sample_predict(self, img_input, a0, c0, start_seq, max_len, units=None, tokenizer=None, temperature=1.0,
                       sample_step=0, top_k=0, top_p=1.0, return_s=True, constraints=None, consensus=None, guidance=None):
        """greedy_predict_attention with the argmax replaced by lc_NIC.sample_choice (lc_NIC.py:571-575:
        tf.random.categorical(log(probs), 1)); ``temperature`` as in ThinkAndTell/evaluate.py:223.  TF's
        sampler cannot be reproduced; the draw is the Philox stream (seed, S_SAMPLE + position, sample_step),
        restated by oracle.ops.sample_rows.  Same return tuple as greedy_predict.

        ``top_k`` (>= 1: only the k most likely tokens) and ``top_p`` (< 1: only the shortest most-likely prefix whose
        mass reaches top_p) filter each draw (tnt_sample_topkp_f32, definition in include/tnt_hip.h; lc_NIC
        select_nucleus2, lc_NIC.py:694-710).  With both at their defaults the draw is the unfiltered one above.  A
        filtered decode is captured and replayed like greedy_predict; sample_step reaches the replay through a device
        word, so every call draws its own stream without a re-capture.
        ``constraints``, ``consensus``, ``guidance`` as in greedy_predict: the draw is from the constrained, mixed or guided
        distribution, which is also what the returned probabilities hold then."""
        top_k, top_p, temperature = check_sampling(top_k, top_p, temperature)
        if top_k == 0 and top_p == 1.0:
            return self.greedy_predict(img_input, a0, c0, start_seq, max_len, units, tokenizer,
                                       _sample=(temperature, int(sample_step)), return_s=return_s, constraints=constraints,
                                       consensus=consensus, guidance=guidance)
        return self.greedy_predict(img_input, a0, c0, start_seq, max_len, units, tokenizer,
                                   _filter=(temperature, top_k, top_p, int(sample_step)), return_s=return_s,
                                   constraints=constraints, consensus=consensus, guidance=guidance)

    def greedy_predict(self, img_input, a0, c0, start_seq, max_len, units=None, tokenizer=None, training=False,
                       _sample=None, return_s=True, _filter=None, constraints=None, consensus=None, guidance=None):
        """lc_NIC.greedy_predict -> greedy_predict_attention (lc_NIC.py:507-508,577-638).
        Returns (words (B,max_len,1) int64, probs (B,max_len,V), alpha (max_len,B,R,1), s (max_len,B,R,A))
        as numpy arrays; the whole decode runs on the device with no per-step host sync.
        ``constraints``, ``consensus``, ``guidance``: model_base.DecodeConstraints, Consensus and Guidance, whose docstrings
        define them.  With consensus (img_input, a0, c0 hold G * M rows, member-major; with n_subjects = S the members are
        the S subject slices and G must be S) words (M, max_len, 1) and probs (M, max_len, V), the mixtures, are per
        image; with guidance words and probs, the guided distributions, are per scan.  alpha and s stay per member row,
        (max_len, G*M, R, ...), under guidance (max_len, 2*B, R, ...) with the scans' rows first."""
        choice, s_all, M = self._decode(img_input, a0, c0, start_seq, max_len, _sample, _filter, return_s, constraints,
                                        consensus, guidance, training)
        ids = choice.ids[:, :M]                        # member 0's rows: every member holds the common word
        out_words = ids.t().contiguous().cpu().numpy().astype(np.int64)[:, :, None]
        out_probs = choice.probs[:, :, :self.V].permute(1, 0, 2).contiguous().cpu().numpy()
        # s (the dropout-free tanh activations, 44 MB at the BASELINE shape) is part of the reference's return tuple but
        # only analysis code reads it: return_s=False skips its device-to-host copy (eval_model does)
        return out_words, out_probs, self.alpha[:max_len].cpu().numpy()[..., None], (s_all.cpu().numpy() if return_s else None)

    greedy_predict_attention = greedy_predict

    def _decode(self, img_input, a0, c0, start_seq, max_len, _sample=None, _filter=None, return_s=True, constraints=None,
                consensus=None, guidance=None, training=False):
        """the decode loop of greedy_predict and sample_predict on the device: returns (the step's choice
        (model_base._TokenChoice: probs, ids), s (max_len, B, R, A) or None, M captions)"""
        cons, (img_input, a0, c0), start, M, G, B, con, _, ckey = self._decode_setup(
            guidance, consensus, constraints, None, img_input, a0, c0, start_seq, max_len, training=training)
        self._stage_inputs((img_input, torch.zeros(B, max_len, dtype=torch.int32), a0, c0))
        # decode buffers are static per (B, max_len) so that the whole loop can be one captured hipGraph
        # (encoder + max_len x {embed, project, attention, LSTM step, head, softmax, argmax}: ~8 launches per token)
        choice = _TokenChoice(self, B, max_len, _filter if _filter is not None else _sample, con, cons)
        choice.start.copy_(start.view(B, 1))
        s_all = None
        if return_s:
            sbufs = self._dec_s
            if (B, max_len) not in sbufs:
                sbufs[B, max_len] = self._f(max_len, B, self.R, self.A)
            s_all = sbufs[B, max_len]

        def run():
            self._encode(B, False)
            words = choice.start
            for i in range(max_len):
                logits = choice.logits(i)
                self._token_step(i, words, B, logits, s_all[i] if return_s else None)     # :596-623
                words = choice.step(i, logits, words)                                              # :627
        key = (B, max_len, bool(return_s)) + ((G,) if cons is not None else ())
        if _filter is not None:     # the stream step is read from the step word on the device: captured like the greedy loop
            self._run_captured(("sample",) + key + tuple(_filter[:3]) + ckey, run)
        elif _sample is None:
            self._run_captured(("greedy",) + key + ckey, run)
        else:                      # the sampling stream step is a launch argument: not captured
            run()
        return choice, s_all, M

    def _mbr_candidate(self, img_input, a0, c0, start_seq, max_len, filt, constraints=None, consensus=None, guidance=None):
        """ModelBase.mbr_decode's candidate decode: sample_predict's (with both filters off the unfiltered draw, as there) or
        (``filt`` None) greedy_predict's, ids left on the device"""
        sample = None
        if filt is not None and filt[1] == 0 and filt[2] == 1.0:
            sample, filt = (filt[0], filt[3]), None
        return self._decode(img_input, a0, c0, start_seq, max_len, sample, filt, False, constraints, consensus, guidance)[0].ids

    # ------------------------------------------------------------------ caption scoring (ModelBase.score_captions)
    def _score_refuse(self):
        if self.S > 1:
            raise NotImplementedError("score_captions is built for one subject: n_subjects > 1 is not supported")
        if self.use_layer_norm:
            raise NotImplementedError("score_captions is not built for the LayerNorm LSTM cell (use_layer_norm=True)")
        if self.grad_sync is not None:
            raise NotImplementedError("score_captions has no data-parallel schedule: score on one device")

    def _score_chain(self, R):
        """the persistent attention -> LSTM chain applies to a scoring pass of R rows"""
        return bool(self._lc_seq_ok() and R <= 128 and self.be.lstm_seq_supported(R, self.U))

    def _score_bufs(self, Rmax, T):
        """decoder buffers of one scoring pass of up to Rmax rows: the gathered region features F and their loop-invariant
        projection P, T-1 attention -> LSTM steps, the head, the kernel's outputs"""
        f, Rg, D, A, U, Et, H, steps = self._f, self.R, self.D, self.A, self.U, self.Et, self.H, T - 1
        # the persistent chain (passes of <= 128 rows) keeps every step's attention and gates, the per-step kernels one slab
        seq_rows = min(Rmax, 128) if self._lc_seq_ok() else 0
        slab = max(Rmax, steps * seq_rows)
        work = f(self.be.lc_seq_fwd_work_floats(seq_rows)) if seq_rows else None
        return dict(cap=torch.zeros(Rmax * T, dtype=torch.int32, device=self.device), F=f(Rmax * Rg * D), P=f(Rmax * Rg * A),
                    text=f(T * Rmax * Et), xz=f(steps * Rmax * 4 * U), hs=f((steps + 1) * Rmax * U),
                    cs=f((steps + 1) * Rmax * U), gates=f(slab * 4 * U), qpre=f(slab * A), alpha=f(slab * Rg), ctx=f(slab * D),
                    ctx_d=f(slab * D), ipre=f(steps * Rmax * H), inter=f(steps * Rmax * H),
                    logits=f(steps * Rmax * self.ldV), tok_lp=f(steps * Rmax), cap_lp=f(Rmax),
                    cap_len=torch.zeros(Rmax, dtype=torch.int32, device=self.device), work=work)

    def _score_shape(self, st, R, T):
        Rg, D, A, U, Et, H, steps = self.R, self.D, self.A, self.U, self.Et, self.H, T - 1
        pre = lambda k, *shape: st[k][:int(np.prod(shape))].view(*shape)
        seq = st["work"] is not None and self._score_chain(R)
        lead = (steps, R) if seq else (R,)
        return dict(cap=pre("cap", R, T), F=pre("F", R, Rg, D), P=pre("P", R * Rg, A), text=pre("text", T * R, Et),
                    xz=pre("xz", steps * R, U, 4), hs=pre("hs", steps + 1, R, U), cs=pre("cs", steps + 1, R, U),
                    gates=pre("gates", *lead, U, 4), qpre=pre("qpre", *lead, A), alpha=pre("alpha", *lead, Rg),
                    ctx=pre("ctx", *lead, D), ctx_d=pre("ctx_d", *lead, D), ipre=pre("ipre", steps * R, H),
                    inter=pre("inter", steps * R, H), logits=pre("logits", steps * R, self.ldV),
                    tok_lp=pre("tok_lp", steps * R), cap_lp=pre("cap_lp", R), cap_len=pre("cap_len", R), seq=seq,
                    work=st["work"])

    def _score_pass(self, B, Cr, T, end_id, v, first):
        """one scoring pass over R = B*Cr decoder rows.  ``first``: the inference encoder of the B staged scans (_encode:
        the normalised region features F and P = LeakyReLU(W1 F + b1)) runs in front.  Then: F, P and the initial state
        gathered to the R rows (the voxel-wide input is never repeated); the Embedding gather and the text half of the
        input projection of the T-1 steps; the attention -> LSTM steps as the persistent chain or per step, in inference
        mode; the two head GEMMs; and tnt_caption_score_f32 on the logits (no softmax launch)."""
        be, a = self.be, self.arena
        Rg, D, A, U, Et, V, ldV = self.R, self.D, self.A, self.U, self.Et, self.V, self.ldV
        R, steps = B * Cr, T - 1
        n = steps * R
        if first:
            self._encode(B, False)
        F, P, hs, cs, xz, cap, rep = v["F"], v["P"], v["hs"], v["cs"], v["xz"], v["cap"], v["rep"]
        be.embedding_fwd(self.F, rep, F, R, 1, Rg * D, Rg * D, B)
        be.embedding_fwd(self.P, rep, P, R, 1, Rg * A, Rg * A, B)
        be.embedding_fwd(self.Hs[0], rep, hs[0], R, 1, U, U, B)
        be.embedding_fwd(self.Cs[0], rep, cs[0], R, 1, U, U, B)
        be.embedding_fwd(a.p("emb_text/embeddings"), cap, v["text"], R, T, Et, Et, V)   # t-major; rows [0, n) are used
        Wl, Ur, bl = a.p("lstm/kernel"), a.p("lstm/recurrent_kernel"), a.p("lstm/bias")
        self.gemm_sk(v["text"], Wl[D:], xz, n, 4 * U, Et, Et, 4 * U, 4 * U)
        att = (a.p("attention/W2/kernel"), a.p("attention/W2/bias"), a.p("attention/V/kernel"), a.p("attention/V/bias"))
        if v["seq"]:
            be.lc_seq_fwd(F, P, *att, v["qpre"], v["alpha"], v["ctx"], v["ctx_d"], None, 0, xz, Wl[:D], Ur, bl, hs, cs,
                          v["gates"], steps, R, Rg, D, A, U, 0.2, 0.0, 0.0, D + Et, self.seed, S_ATTN, S_LSTM_IN,
                          self.drop_step, v["work"], self.seq_sync, self._guard_out(), out_drop=None)
        else:
            for i in range(steps):
                be.attention_step_fwd(hs[i], F, P, *att, v["qpre"], v["alpha"], v["ctx"], v["ctx_d"], None, R, Rg, D, A, U,
                                      0.2, 0.0, 0.0, D + Et, self.seed, S_ATTN + i, S_LSTM_IN + i, 0, self.drop_step,
                                      keep4=None)
                be.lstm_step_fwd(xz[i * R:(i + 1) * R], hs[i], cs[i], Ur, v["ctx_d"], Wl[:D], D, None, 0, 0, None,
                                 hs[i + 1], cs[i + 1], None, v["gates"], R, U, xz_bias=bl)
        self._head_inter(hs[1:].view(n, U), v["inter"], n, v["ipre"])
        self._head_out(v["inter"], v["logits"], n)
        be.caption_score(v["logits"], ldV, V, cap, T, steps, R, end_id, v["tok_lp"], v["cap_lp"], v["cap_len"])

    def beam_search(self, img_input, a0, c0, start_seq, max_len, beam_width=5, end_id=-1, units=None, tokenizer=None,
                    length_penalty=0.0, constraints=None, consensus=None, diversity=None, guidance=None):
        """Beam search over the attention decoder.  The reference only sketches it (lc_NIC.beam_search / _beam_search,
        lc_NIC.py:640-692, recurse without returning; ThinkAndTell/evaluate.py:203-228 stops after one expansion), so
        the definition is this library's: standard log-probability beam search of width ``beam_width`` with the greedy
        decoder's step (lc_NIC.py:596-632), no length normalisation by default; a beam that emits ``end_id`` (the tokenizer's
        '<end>' index; -1 = never) is finished and pads with 0.  Returns (sequences (B, k, max_len) int64, best first;
        scores (B, k) float32 = sum of log-probabilities).  The whole search runs on the device: per token one
        expansion launch (tnt_beam_topk_f32) and row gathers of the LSTM state by parent beam; the paths are
        back-tracked on the host at the end.  Restated by oracle.models.LcNIC.beam_search.
        ``length_penalty`` > 0 reorders the k results by score / ((5 + L) / 6) ** length_penalty and returns that key as
        the scores (model_base.length_normalise); the search itself is unchanged.
        ``constraints``, ``consensus``, ``diversity``, ``guidance``: model_base.DecodeConstraints, Consensus, BeamDiversity
        and Guidance, whose docstrings define them.  Here the expansion under diversity is tnt_beam_step_diverse_f32 with
        U = 0 (the state gathers stay).  With consensus the inputs hold G * M rows, member-major (with n_subjects = S: the
        S subject slices), start_seq M entries, and sequences and scores are per image."""
        length_penalty = check_length_penalty(length_penalty)
        be = self.be
        k = int(beam_width)
        # M captions: the expansion runs on M * k rows; B = G * M staged scans: the decoder runs B * k rows, [G][M][k]
        cons, (img_input, a0, c0), start, M, _, B, con, div, _ = self._decode_setup(
            guidance, consensus, constraints, diversity, img_input, a0, c0, start_seq, max_len, k, end_id)
        end_id, Bk = int(end_id), B * k
        rep = lambda t: np.repeat(np.asarray(t), k, axis=0)
        x = img_input.cpu().numpy() if isinstance(img_input, torch.Tensor) else np.asarray(img_input)
        self._stage_inputs((rep(x), torch.zeros(Bk, max_len, dtype=torch.int32), rep(np.asarray(a0)), rep(np.asarray(c0))))
        U, V, ldV = self.U, self.V, self.ldV
        probs = self.logits[:Bk]
        hg, cg = self._f(Bk, U), self._f(Bk, U)
        # the expansion launch: tnt_beam_topk_f32, or with diversity tnt_beam_step_diverse_f32 without its reorder (U = 0)
        if div is None:
            expand = lambda p, score_in, fin_in, *outs: be.beam_topk(p, score_in, fin_in, M, V, ldV, k, end_id, *outs)
        else:
            expand = lambda p, score_in, fin_in, *outs: be.beam_step_diverse(
                p, ldV, score_in, fin_in, M, V, k, end_id, *outs, None, None, 0, 0, None, None, *div)
        beam = _BeamDecode(self, M, k, max_len, end_id, expand, con, cons, div)
        self._encode(Bk, False)
        words = start.repeat_interleave(k).view(Bk, 1)
        for i in range(max_len):
            self._token_step(i, words, Bk, probs)
            words, par = beam.step(i, probs)
            # the surviving beams continue from their parents' LSTM state (row gather by parent)
            be.embedding_fwd(self.Hs[i + 1], par, hg, Bk, 1, U, U, Bk)
            be.embedding_fwd(self.Cs[i + 1], par, cg, Bk, 1, U, U, Bk)
            self.Hs[i + 1].copy_(hg)
            self.Cs[i + 1].copy_(cg)
        return beam.finish(length_penalty)
