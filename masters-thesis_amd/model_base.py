"""Keras-style model surface shared by the NIC variants.

Mirrors what AttemptFour/main.py and eval.py call on a ``tf.keras.Model``
(SURVEY.md 8b): ``compile``, ``__call__``, ``fit``, ``train_step``, ``test_step``,
``save_weights`` / ``load_weights(by_name, skip_mismatch)``, ``summary``,
``get_layer(name).get_weights/set_weights``, ``optimizer.lr``, ``trainable_variables``,
``losses`` -- on top of the HIP kernel backend.  Host code here only sequences kernel
launches and owns buffers; it contains no arithmetic of the hot path.
"""
import time
from collections import OrderedDict
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from . import compat, ops
from .optimizers import (Adam, check_class_weight, loss_class_weight, loss_distillation, loss_focal_gamma, loss_label_smoothing,
                         loss_normalise,
                         loss_unlikelihood, optimizer_average, optimizer_schedule, check_global_clipnorm,
                         check_gradient_accumulation_steps, check_weight_decay, weight_decay_table)

# dropout site ids of the Philox stream (shared with oracle/models.py)
S_IN, S_FEAT, S_TEXT, S_OUT = 1, 2, 3, 5
S_ATTN, S_LSTM_IN, S_LSTM_OUT = 16, 48, 80
S_SAMPLE = 112          # + decode position: categorical-sampling stream of sample_predict
# + token position j (< 32): scheduled sampling's coin and draw streams (nic.NIC and lc_nic.NIC(scheduled_sampling=...));
# after lc_nic.S_NOUT = 144 + step
S_SS_COIN, S_SS_DRAW = 176, 208
SS_MAX_POSITIONS = 32
S_SCST_LAST = 240       # self-critical rollouts: the draw of the last token position (nic.NIC(self_critical=...))
# the training-time input corruption of nic.NIC / lc_nic.NIC (tnt_input_corrupt_f32): element b decides scan row b,
# element b * T + t the fed caption token (b, t)
S_SCAN_DROP, S_WORD_DROP = 241, 242
BN_EPS, BN_MOMENTUM = 1e-3, 0.99


SCORE_LOGITS_BYTES = 256 << 20      # score_captions: default bound on the logits of one decoder pass (sets max_rows)


class AttentionCoverage:
    """The coverage ("doubly stochastic attention") penalty of Show, Attend and Tell (Xu et al. 2015, section 4.2.1) for
    the train_step of lc_nic.NIC; the definition is tnt_attention_coverage_f32's (include/tnt_hip.h).  With alpha [T][B][R]
    the attention weights of a step's T decoder positions,
      axis="time"  (Xu et al.):  s[b][r] = sum_t alpha[t][b][r]
      axis="batch" (the reference's own line, lc_NIC.py:365-367, whose axis=1 is the batch axis): s[t][r] = sum_b alpha[t][b][r]
    coverage = mean (1 - s)^2, and the step differentiates CE + L2 + weight * coverage.  The step's metrics gain the
    unweighted ``coverage``; ``loss`` stays the cross-entropy.  weight = 0 is the model without the term.
    Bad parameters raise ValueError here, before any launch."""

    AXES = ("time", "batch")

    def __init__(self, weight, axis="time"):
        if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not np.isfinite(weight):
            raise ValueError(f"attention coverage weight must be a finite number, got {weight!r}")
        if weight < 0:
            raise ValueError(f"attention coverage weight must be >= 0, got {weight!r}")
        if axis not in self.AXES:
            raise ValueError(f"attention coverage axis must be one of {self.AXES}, got {axis!r}")
        self.weight, self.axis = float(weight), axis

    @property
    def axis_id(self):
        """the kernel's axis argument: 0 = time, 1 = batch"""
        return self.AXES.index(self.axis)

    @property
    def key(self):
        """what a recorded plan or a captured graph of the step depends on"""
        return ("coverage", self.weight, self.axis)

    def rows(self, T, B):
        """the number of sums per region: B over time, T over the batch"""
        return B if self.axis == "time" else T

    def coef(self, T, B, R):
        """2 weight / N, the factor of (s - 1) in the gradient"""
        return 2.0 * self.weight / (self.rows(T, B) * R)

    def strides(self, R):
        """(ext_ts, ext_bs): the element strides of the gradient rider between steps and between samples"""
        return (0, R) if self.axis == "time" else (R, 0)

    def __eq__(self, other):
        return isinstance(other, AttentionCoverage) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return f"AttentionCoverage(weight={self.weight!r}, axis={self.axis!r})"


class LearnedInitState:
    """The learned initial LSTM state of Show, Attend and Tell (Xu et al. 2015, section 3.1.2) for lc_nic.NIC; the reference
    names it learn_init_state (lc_NIC.py:169-173: "init the LSTM h,c state as MLP(mean(features))") and never builds the two
    layers it reads, so the definition is tnt_init_state_fwd_f32's (include/tnt_hip.h).  With F [B][R][D] the region features
    the attention reads -- behind BatchNorm / LayerNorm and the feature Dropout, in training and inference mode alike --
      m = mean_r F,   h0 = tanh(m Wh + bh),   c0 = tanh(m Wc + bc)
    Wh, bh are the layer ``hidden_init`` (kernel (D, U), bias (U,)), Wc, bc the layer ``carry_init``: Glorot-uniform
    kernels, zero biases.  ``reg`` is the L2 coefficient of both kernels (part of the ``L2`` metric and of the gradient).
    The ``a0`` / ``c0`` every call still takes are shape-checked and their values are not used."""

    def __init__(self, reg=0.0):
        if isinstance(reg, bool) or not isinstance(reg, (int, float, np.integer, np.floating)) or not np.isfinite(reg):
            raise ValueError(f"the L2 coefficient of the learned initial state must be a finite number, got {reg!r}")
        if reg < 0:
            raise ValueError(f"the L2 coefficient of the learned initial state must be >= 0, got {reg!r}")
        self.reg = float(reg)

    LAYERS = ("hidden_init", "carry_init")

    @classmethod
    def from_config(cls, value):
        """the config key ``learn_init_state``: true, false / null (off), or {reg: <float>}"""
        if value is None or value is False:
            return None
        if value is True:
            return cls()
        if not isinstance(value, dict) or not set(value) <= {"reg"}:
            raise ValueError(f"learn_init_state must be true, false or a mapping with reg, got {value!r}")
        return cls(value.get("reg", 0.0))

    def __eq__(self, other):
        return isinstance(other, LearnedInitState) and self.reg == other.reg

    def __hash__(self):
        return hash(("init_state", self.reg))

    def __repr__(self):
        return f"LearnedInitState(reg={self.reg!r})"


class SemanticTarget:
    """The sentence-embedding target of nic.NIC: the reference hands every model the caption's Universal Sentence Encoder
    ("GUSE") vector as a fifth input (data_generator_guse.py's guse_key, lc_NIC.train_step's ``guse = data[0][-1]``) and
    defines cosine_loss = 1 - cosine_similarity (lc_NIC.py:488-502) without ever applying it; Model/guse.py names the use: "a
    model that linearly maps the brain betas to an embedding vector.  Then KNN is used to find a known GUSE vector".  The
    definition is tnt_cosine_loss_f32's (include/tnt_hip.h).  With x_b the feature row exactly as the first LSTM step receives
    it (behind BatchNorm and, in training, the feature step's LSTM-input Dropout), g_b the target and the layer ``guse_out``
    (kernel (E, dim) Glorot-uniform, L2 ``reg``; bias (dim,) zeros):
      z_b = x_b W + bias,   zn = z / sqrt(max(sum z^2, 1e-12)),   gn likewise,   semantic = mean_b (1 - sum zn gn)
    train_step differentiates CE + L2 + ``weight`` * semantic and reports the unweighted value as the metric ``semantic``;
    ``loss`` stays the cross-entropy.  A target row of all zeros (the reference's missing embedding) gives loss 1 and no
    gradient, and counts in the mean.  data[0] is then (betas, cap, a0, c0, guse) with guse (B, dim) float32.

    ``loss="contrastive"`` trains the same layer with the CLIP-style loss of the fMRI-decoding literature instead: in-batch
    negatives, a ``temperature``, both directions (``symmetric``) and, with ``soft_temperature``, soft targets, so that two
    captions of similar images are not hard negatives.  The definition is tnt_contrastive_loss_f32's (include/tnt_hip.h),
    with eps = 1e-12:
      iz_i = 1/sqrt(max(sum z_i^2, eps)),  ig_j likewise,  zn = z*iz, gn = g*ig
      valid_j = (sum g_j^2 > eps)                        an all-zero target is the reference's missing embedding
      Bv = number of valid rows
      L_ij = (zn_i . gn_j) / temperature                 over valid i, j only
      Q_ij = [i == j]                                    (hard: soft_temperature=None)
      Q_i. = softmax_j( (gn_i . gn_j) / soft_temperature ) over valid j   (soft)
      lr_i = - sum_j Q_ij log softmax_j(L_i.)_j          scan -> caption
      lc_i = - sum_j Q_ij log softmax_j(L_.i)_j          caption -> scan: column i of L, softmax over rows
      row_i = symmetric ? 0.5 (lr_i + lc_i) : lr_i       0 for an invalid row
      semantic = sum_i row_i / max(Bv, 1)
      semantic_top1 = sum_i [valid_i and (first argmax over valid j of L_ij) == i] / max(Bv, 1)
    train_step differentiates CE + L2 + ``weight`` * semantic and reports the unweighted ``semantic`` and ``semantic_top1``;
    test_step reports them too.  An invalid row has no gradient and takes no part in any softmax; Bv = 0 and a batch of one
    give 0.  ``semantic_top1`` rides in slot 5 of ``met`` (TOP1_SLOT): ModelBase.DISTILL_KL's, which cannot be live here
    because distillation is refused beside ``semantic`` (compat).  Under ``loss="cosine"``, the default, ``temperature``,
    ``symmetric`` and ``soft_temperature`` are ignored and normalised to their defaults: the object equals and hashes as the
    three-argument one."""

    LOSSES = ("cosine", "contrastive")

    def __init__(self, dim=512, weight=1.0, reg=0.0, loss="cosine", temperature=0.07, symmetric=True, soft_temperature=None):
        num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or not 1 <= dim <= 2048:
            raise ValueError(f"the semantic target's dim must be an integer in [1, 2048] (tnt_cosine_loss_f32), got {dim!r}")
        if not num(weight) or weight < 0:
            raise ValueError(f"the semantic target's weight must be a finite number >= 0, got {weight!r}")
        if not num(reg) or reg < 0:
            raise ValueError(f"the semantic target's L2 coefficient (reg) must be a finite number >= 0, got {reg!r}")
        if not isinstance(loss, str) or loss not in self.LOSSES:
            raise ValueError(f"the semantic target's loss must be \"cosine\" or \"contrastive\", got {loss!r}")
        if not num(temperature) or temperature <= 0:
            raise ValueError(f"the semantic target's temperature must be a finite number > 0, got {temperature!r}")
        if not isinstance(symmetric, (bool, np.bool_)):
            raise ValueError(f"the semantic target's symmetric must be a bool, got {symmetric!r}")
        if soft_temperature is not None and (not num(soft_temperature) or soft_temperature <= 0):
            raise ValueError(f"the semantic target's soft_temperature must be None or a finite number > 0, got "
                             f"{soft_temperature!r}")
        self.dim, self.weight, self.reg, self.loss = int(dim), float(weight), float(reg), loss
        if loss == "cosine":                # the contrastive fields do not exist for the cosine loss
            temperature, symmetric, soft_temperature = 0.07, True, None
        self.temperature, self.symmetric = float(temperature), bool(symmetric)
        self.soft_temperature = None if soft_temperature is None else float(soft_temperature)

    LAYER = "guse_out"
    SLOT = 6                # slot of ``met`` that carries the unweighted mean (free in nic.NIC)
    TOP1_SLOT = 5           # ... and semantic_top1 (loss="contrastive"): DISTILL_KL's, refused beside semantic
    KEYS = ("dim", "weight", "reg", "loss", "temperature", "symmetric", "soft_temperature")

    @property
    def contrastive(self):
        return self.loss == "contrastive"

    @classmethod
    def from_config(cls, value):
        """the config key ``semantic``: null (off) or {dim: , weight: , reg: , loss: , temperature: , symmetric: ,
        soft_temperature: }, each optional"""
        if value is None:
            return None
        if not isinstance(value, dict) or not set(value) <= set(cls.KEYS):
            raise ValueError(f"semantic must be a mapping with dim, weight, reg, loss, temperature, symmetric and "
                             f"soft_temperature, got {value!r}")
        return cls(**value)

    def _key(self):
        base = (self.dim, self.weight, self.reg)
        return base if self.loss == "cosine" else base + (self.loss, self.temperature, self.symmetric, self.soft_temperature)

    def __eq__(self, other):
        return isinstance(other, SemanticTarget) and self._key() == other._key()

    def __hash__(self):
        return hash(("semantic",) + self._key())

    def __repr__(self):
        base = f"SemanticTarget(dim={self.dim!r}, weight={self.weight!r}, reg={self.reg!r}"
        if self.loss == "cosine":
            return base + ")"
        return base + (f", loss={self.loss!r}, temperature={self.temperature!r}, symmetric={self.symmetric!r}, "
                       f"soft_temperature={self.soft_temperature!r})")


class ScheduledSampling:
    """Scheduled sampling (Bengio et al. 2015) for the train_step of nic.NIC and lc_nic.NIC; the definitions are
    tnt_scheduled_feedback_f32's and tnt_scheduled_feedback2_f32's (include/tnt_hip.h).  At each step, each caption row is
    fed the model's own token with probability p, the ground truth otherwise; p grows with i, the updates applied so far
    (the model's device counter adam_t):
      ScheduledSampling.linear(p0, slope, p_max=1.0):  p = clip(p0 + slope * i, 0, p_max)   (constant p: slope = 0)
      ScheduledSampling.inverse_sigmoid(k, p_max=1.0): p = p_max * (1 - k / (k + exp(i / k))), k >= 1
    mode "greedy" feeds the argmax of the step's logits, "sample" a categorical draw from them (temperature 1).
    p is computed in float64 and rounded to float32, on the device by the kernel and on the host by ``p(i)``.
    Bad parameters raise ValueError here, before any launch."""

    KINDS = ("linear", "inverse_sigmoid")
    MODES = ("greedy", "sample")

    def __init__(self, kind, mode="greedy", p0=0.0, slope=0.0, p_max=1.0, k=1.0):
        if kind not in self.KINDS:
            raise ValueError(f"scheduled sampling kind must be one of {self.KINDS}, got {kind!r}")
        if mode not in self.MODES:
            raise ValueError(f"scheduled sampling mode must be one of {self.MODES}, got {mode!r}")

        def num(name, v):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"scheduled sampling {name} must be a finite number, got {v!r}")
            return float(v)
        p0, slope, p_max, k = num("p0", p0), num("slope", slope), num("p_max", p_max), num("k", k)
        if not 0.0 <= p_max <= 1.0:
            raise ValueError(f"scheduled sampling p_max must be in [0, 1], got {p_max!r}")
        if kind == "linear" and not 0.0 <= p0 <= 1.0:
            raise ValueError(f"scheduled sampling p0 must be in [0, 1], got {p0!r}")
        if kind == "inverse_sigmoid" and not k >= 1.0:
            raise ValueError(f"scheduled sampling k must be >= 1, got {k!r}")
        self.kind, self.mode, self.p0, self.slope, self.p_max, self.k = kind, mode, p0, slope, p_max, k

    @classmethod
    def linear(cls, p0, slope, p_max=1.0, mode="greedy"):
        return cls("linear", mode, p0=p0, slope=slope, p_max=p_max)

    @classmethod
    def inverse_sigmoid(cls, k, p_max=1.0, mode="greedy"):
        return cls("inverse_sigmoid", mode, k=k, p_max=p_max)

    @property
    def kind_id(self):
        return self.KINDS.index(self.kind)

    @property
    def mode_id(self):
        return self.MODES.index(self.mode)

    def params(self):
        """the kernel's float64 parameter triple"""
        return (self.p0, self.slope, self.p_max) if self.kind == "linear" else (self.k, 0.0, self.p_max)

    def p(self, i):
        """p after i updates, as the kernel computes it: float64, rounded to float32"""
        i = float(int(i))
        if self.kind == "linear":
            return np.float32(min(max(self.p0 + self.slope * i, 0.0), self.p_max))
        with np.errstate(over="ignore"):
            e = float(np.exp(np.float64(i / self.k)))
        return np.float32(self.p_max * (1.0 - self.k / (self.k + e)))

    def __repr__(self):
        if self.kind == "linear":
            return f"ScheduledSampling.linear(p0={self.p0}, slope={self.slope}, p_max={self.p_max}, mode={self.mode!r})"
        return f"ScheduledSampling.inverse_sigmoid(k={self.k}, p_max={self.p_max}, mode={self.mode!r})"


class SelfCritical:
    """Self-critical sequence training (Rennie et al. 2017) for nic.NIC's train_step (nic.NIC.train_step_scst): per scan
    K = ``n_samples`` captions are sampled from the model (temperature 1), each scored by ``reward`` against the scan's
    references, and the loss (1/R) sum_r -(reward_r - baseline_r) sum_t m_rt log p(w_rt) (R = B*K, m: the tokens up to and
    including the first terminator) is minimised; its definition on the device is tnt_scst_cce_f32's (include/tnt_hip.h).
      end_id     the tokenizer's <end> index; a caption ends at its first end_id or 0
      n_samples  K sampled captions per scan, 1..16
      baseline   "greedy": the reward of the model's inference-mode greedy caption of the scan; "mean": the mean reward of
                 the scan's other K-1 samples (K >= 2, no decode)
      reward     "cider-d" (evaluate.CiderD), "bleu4" (evaluate.sentence_bleu, weights (0.25,)*4, method 1), "rouge-l"
                 (evaluate.rouge_l at beta 1.2: the reward that credits in-order word matches with gaps; needs no corpus)
                 or a callable (candidate_ids, reference_id_lists) -> float
      corpus     tokenised reference captions, one list of references per scan: CIDEr-D's document frequencies; None takes
                 them from each batch's references
      score_on   "host": the sampled ids visit the host in the middle of the step and ``reward`` is scored in Python;
                 "device": one tnt_caption_reward_f32 launch (tnt_caption_rouge_f32 for "rouge-l") between the rollout and
                 the update scores them (definition: include/tnt_hip.h), no id and no reward crosses the bus and the host
                 does not wait.  On the device ``reward`` is one of the names, "cider-d" needs ``corpus`` (evaluate.RewardTable holds its document
                 frequencies), a step takes at most 8 references per scan of at most 64 tokens, and a reference is cut at
                 its first end_id or 0 like a candidate
    Bad arguments raise ValueError here, before any launch."""

    BASELINES = ("greedy", "mean")
    REWARDS = ("cider-d", "bleu4", "rouge-l")
    SCORE_ON = ("host", "device")

    def __init__(self, end_id, n_samples=1, baseline="greedy", reward="cider-d", corpus=None, score_on="host"):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not is_int(end_id) or end_id < 1:
            raise ValueError(f"self-critical end_id must be an int >= 1 (the <end> index), got {end_id!r}")
        if not is_int(n_samples) or not 1 <= n_samples <= 16:
            raise ValueError(f"self-critical n_samples must be an int in [1, 16], got {n_samples!r}")
        if baseline not in self.BASELINES:
            raise ValueError(f"self-critical baseline must be one of {self.BASELINES}, got {baseline!r}")
        if baseline == "mean" and n_samples < 2:
            raise ValueError("self-critical baseline 'mean' needs n_samples >= 2 (the other samples of the scan)")
        if not (callable(reward) or (isinstance(reward, str) and reward in self.REWARDS)):
            raise ValueError(f"self-critical reward must be one of {self.REWARDS} or a callable, got {reward!r}")
        if not (isinstance(score_on, str) and score_on in self.SCORE_ON):
            raise ValueError(f"self-critical score_on must be one of {self.SCORE_ON}, got {score_on!r}")
        if score_on == "device":
            if not isinstance(reward, str):
                raise ValueError(f"score_on='device' scores {self.REWARDS} only: a callable reward runs on the host")
            if reward == "cider-d" and corpus is None:
                raise ValueError("score_on='device' with reward 'cider-d' needs corpus=: the batch-local document "
                                 "frequencies of corpus=None would have to be rebuilt on the host every step")
        if corpus is not None:
            try:
                corpus = [[list(r) for r in doc] for doc in corpus]
            except TypeError:
                raise ValueError("self-critical corpus must be None or a list of documents, each a list of tokenised "
                                 "references") from None
        self.end_id, self.n_samples, self.baseline, self.reward, self.corpus = int(end_id), int(n_samples), baseline, reward, corpus
        self.score_on = score_on
        self._cider = self.table = None
        if reward == "cider-d":
            from .evaluate import CiderD
            self._cider = CiderD(corpus)
        if score_on == "device" and reward == "cider-d":
            from .evaluate import RewardTable
            self.table = RewardTable(self.corpus)      # the kernel's view of _cider's frequencies, uploaded on first use

    def truncate(self, ids):
        """the tokens of a caption before its first terminator (end_id or 0)"""
        out = []
        for w in ids:
            w = int(w)
            if w == 0 or w == self.end_id:
                break
            out.append(w)
        return out

    def counted(self, ids):
        """the number of token positions the loss counts: up to and including the first terminator"""
        for i, w in enumerate(ids):
            if int(w) == 0 or int(w) == self.end_id:
                return i + 1
        return len(ids)

    def scores(self, candidates, references):
        """candidates: one list of token-id sequences per scan, references: one list of references per scan ->
        one float64 array of rewards per scan"""
        if self._cider is not None:
            return self._cider.batch_scores(candidates, references)
        if self.reward == "bleu4":
            from .evaluate import sentence_bleu
            fn = lambda c, refs: sentence_bleu(refs, c, weights=(0.25,) * 4) if refs else 0.0
        elif self.reward == "rouge-l":
            from .evaluate import rouge_l
            fn = lambda c, refs: rouge_l(refs, c)
        else:
            fn = self.reward
        return [np.array([float(fn(c, refs)) for c in cands], np.float64) for cands, refs in zip(candidates, references)]

    def advantages(self, samples, references, greedy=None):
        """samples: (B*K, T) sampled ids w_1..w_T (row b*K + k: sample k of scan b); references: B lists of references;
        greedy: (B, T) greedy ids (baseline "greedy").  Returns float64 arrays (adv, reward, baseline, counted), each (B*K,)."""
        samples = np.asarray(samples)
        K = self.n_samples
        B = samples.shape[0] // K
        if samples.shape[0] != B * K or len(references) != B:
            raise ValueError(f"{samples.shape[0]} samples and {len(references)} reference lists for n_samples = {K}")
        refs = [[list(r) for r in doc] for doc in references]
        cands = [[self.truncate(samples[b * K + k]) for k in range(K)] for b in range(B)]
        if self.baseline == "greedy":
            if greedy is None:
                raise ValueError("baseline 'greedy' needs the greedy captions")
            g = np.asarray(greedy)
            cands = [c + [self.truncate(g[b])] for b, c in enumerate(cands)]
        sc = self.scores(cands, refs)
        reward = np.concatenate([s[:K] for s in sc])
        if self.baseline == "greedy":
            base = np.repeat(np.array([s[K] for s in sc]), K)
        else:
            r = reward.reshape(B, K)
            base = ((r.sum(1, keepdims=True) - r) / (K - 1)).reshape(-1)
        counted = np.array([self.counted(row) for row in samples], np.float64)
        return reward - base, reward, base, counted

    def __repr__(self):
        return (f"SelfCritical(end_id={self.end_id}, n_samples={self.n_samples}, baseline={self.baseline!r}, "
                f"reward={self.reward!r}, corpus={'None' if self.corpus is None else f'<{len(self.corpus)} documents>'}"
                + (f", score_on={self.score_on!r})" if self.score_on != "host" else ")"))


class MBR:
    """Minimum Bayes risk decoding (Eikema & Aziz 2020, sampling-based), for ``mbr_decode`` of nic.NIC and lc_nic.NIC: per
    scan ``n_samples`` captions are drawn from the model, and the candidate with the highest expected utility against
    those samples is returned -- the caption the model's distribution agrees on, where beam search and the greedy decode
    return its mode and a sampled decode one noisy draw.  The definition on the device is tnt_mbr_select_f32's
    (include/tnt_hip.h).
      end_id          the tokenizer's <end> index; a caption ends at its first end_id or 0
      n_samples       N sampled captions per scan: the pseudo-references, and hypotheses too
      utility         "ngram-f": the mean over k = 1..order of the F1 of the clipped k-gram matches (symmetric); "bleu":
                      evaluate.sentence_bleu([reference], hypothesis, weights=(1/order,)*order), method-1 smoothing
      order           the longest n-gram, 1..4
      include_greedy  the greedy caption is one more hypothesis (never a reference): n_samples + include_greedy <= 64
      temperature, top_k, top_p   the filters of every draw, as sample_predict takes them
    Bad arguments raise ValueError here, before any launch."""

    UTILITIES = ("ngram-f", "bleu")
    MAX_CANDIDATES = 64
    MAX_LEN = 64
    MAX_ORDER = 4

    def __init__(self, end_id, n_samples=16, utility="ngram-f", order=4, include_greedy=True, temperature=1.0, top_k=0,
                 top_p=1.0):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not is_int(end_id) or end_id < 1:
            raise ValueError(f"MBR end_id must be an int >= 1 (the <end> index), got {end_id!r}")
        if not isinstance(include_greedy, (bool, np.bool_)):
            raise ValueError(f"MBR include_greedy must be a bool, got {include_greedy!r}")
        if not is_int(n_samples) or n_samples < 1 or n_samples + int(include_greedy) > self.MAX_CANDIDATES:
            raise ValueError(f"MBR n_samples must be an int >= 1 with n_samples + include_greedy <= {self.MAX_CANDIDATES}, got "
                             f"{n_samples!r} (include_greedy = {include_greedy})")
        if not (isinstance(utility, str) and utility in self.UTILITIES):
            raise ValueError(f"MBR utility must be one of {self.UTILITIES}, got {utility!r}")
        if not is_int(order) or not 1 <= order <= self.MAX_ORDER:
            raise ValueError(f"MBR order must be an int in [1, {self.MAX_ORDER}], got {order!r}")
        self.top_k, self.top_p, self.temperature = check_sampling(top_k, top_p, temperature)
        self.end_id, self.n_samples, self.utility, self.order = int(end_id), int(n_samples), utility, int(order)
        self.include_greedy = bool(include_greedy)

    @property
    def kind(self):
        return self.UTILITIES.index(self.utility)

    @property
    def n_candidates(self):
        return self.n_samples + int(self.include_greedy)

    def __repr__(self):
        return (f"MBR(end_id={self.end_id}, n_samples={self.n_samples}, utility={self.utility!r}, order={self.order}, "
                f"include_greedy={self.include_greedy}, temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p})")


class DecodeConstraints:
    """Constraints on caption decoding, for the ``constraints=`` keyword of greedy_predict, sample_predict and beam_search
    of nic.NIC and lc_nic.NIC; applied to each step's logits on the device, in front of the softmax, from the tokens the
    row's path has chosen so far (the start token is not among them).  The definition is tnt_decode_constrain_f32's
    (include/tnt_hip.h):
      repetition_penalty    theta >= 1 (1: off): the logit of every token of the history is divided by theta if positive,
                            multiplied by it otherwise, once per distinct token
      no_repeat_ngram_size  n >= 0 (0: off): a token that would complete an n-gram the history already holds is banned
      min_length            m >= 0: ``end_id`` is banned at positions 0 .. m-1
      bad_ids               up to 64 token ids banned at every step (<unk>, <pad>, <start>, ...)
      end_id                the tokenizer's <end> index for min_length; -1: beam_search's own end_id
    A banned token has probability exactly 0.  Bad values raise ValueError here, before any launch; what depends on the
    model or the call (vocabulary size, max_len, beam width) is checked by the decode.
    The decode issues one tnt_decode_constrain_f32 launch per token; the probabilities it returns are the constrained
    distributions, and a sampled decode draws from them.  beam_search constrains each live beam row's logits from the
    row's own path (the launch also carries the history across the beam reorder), so its scores are sums of constrained
    log-probabilities; min_length uses the search's ``end_id`` unless the object names its own (the two must agree).
    None or a neutral object: the decode as it is without the keyword."""

    MAX_LEN = 64        # the kernel holds one history token per lane
    MAX_BAD = 64

    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, bad_ids=(), end_id=-1):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        th = repetition_penalty
        if isinstance(th, bool) or not isinstance(th, (int, float, np.integer, np.floating)) or not np.isfinite(th) or th < 1:
            raise ValueError(f"repetition_penalty must be a finite number >= 1 (1: off), got {th!r}")
        if float(th) > float(np.finfo(np.float32).max):
            raise ValueError(f"repetition_penalty must be finite in float32, got {th!r}")
        if not is_int(no_repeat_ngram_size) or no_repeat_ngram_size < 0:
            raise ValueError(f"no_repeat_ngram_size must be an int >= 0 (0: off), got {no_repeat_ngram_size!r}")
        if not is_int(min_length) or min_length < 0:
            raise ValueError(f"min_length must be an int >= 0, got {min_length!r}")
        if not is_int(end_id) or end_id < -1:
            raise ValueError(f"end_id must be an int >= -1 (-1: beam_search's end_id), got {end_id!r}")
        try:
            bad = tuple(bad_ids)
        except TypeError:
            raise ValueError(f"bad_ids must be a sequence of token ids, got {bad_ids!r}") from None
        if not all(is_int(v) and v >= 0 for v in bad):
            raise ValueError(f"bad_ids must be ints >= 0, got {bad_ids!r}")
        if len(bad) > self.MAX_BAD:
            raise ValueError(f"at most {self.MAX_BAD} bad_ids, got {len(bad)}")
        self.repetition_penalty, self.no_repeat_ngram_size, self.min_length = float(th), int(no_repeat_ngram_size), int(min_length)
        self.bad_ids, self.end_id = tuple(int(v) for v in bad), int(end_id)

    @property
    def neutral(self):
        """every rule is off: the decode runs as without constraints"""
        return (np.float32(self.repetition_penalty) == 1 and self.no_repeat_ngram_size == 0 and self.min_length == 0
                and not self.bad_ids)

    def __repr__(self):
        return (f"DecodeConstraints(repetition_penalty={self.repetition_penalty}, no_repeat_ngram_size="
                f"{self.no_repeat_ngram_size}, min_length={self.min_length}, bad_ids={self.bad_ids}, end_id={self.end_id})")


class _ConstrainedDecode:
    """The host part of a constrained decode over ``rows`` rows (ModelBase._constrain): the ping-pong history buffers and
    the bad_ids buffer on the device, the per-step launch, and the suffix of the capture key."""

    def __init__(self, model, c, rows, max_len, end_id):
        bufs = model._decode_bufs("_con_bufs")
        if (rows, max_len) not in bufs:
            bufs[rows, max_len] = torch.zeros(2, rows, max_len, dtype=torch.int32, device=model.device)
        if "bad" not in bufs:
            bufs["bad"] = torch.zeros(DecodeConstraints.MAX_BAD, dtype=torch.int32, device=model.device)
        self.be, self.V, self.rows, self.ldh = model.be, model.V, rows, max_len
        self.hist, self.bad = bufs[rows, max_len], bufs["bad"]
        # the list reaches a replay through the buffer: only its length is in the capture key.  One buffer per model, written
        # here alone and in stream order; an unchanged list is not copied again (the copy is a synchronous one from pageable memory)
        if c.bad_ids and bufs.get("bad_ids") != c.bad_ids:
            self.bad[:len(c.bad_ids)].copy_(torch.tensor(c.bad_ids, dtype=torch.int32))
            bufs["bad_ids"] = c.bad_ids
        self.theta, self.n, self.m, self.end_id, self.n_bad = c.repetition_penalty, c.no_repeat_ngram_size, c.min_length, end_id, len(c.bad_ids)
        self.key = ("constrain", self.theta, self.n, self.m, self.end_id, self.n_bad)

    def step(self, i, logits, ld, last_token, parent=None, fin=None):
        """decode step i: logits [rows][ld] in place; last_token / parent: what step i-1 chose (None at i = 0; parent None:
        every row continues itself); fin: the finished flags the step's expansion reads.  hist[i & 1] then holds the rows'
        histories h_0 .. h_{i-1}."""
        self.be.decode_constrain(logits, ld, self.V, self.rows, i, self.hist[(i & 1) ^ 1], self.hist[i & 1], self.ldh,
                                 last_token, parent, fin, self.theta, self.n, self.m, self.end_id,
                                 self.bad if self.n_bad else None, self.n_bad)


class Consensus:
    """Consensus decoding, for the ``consensus=`` keyword of greedy_predict, sample_predict and beam_search of nic.NIC and
    lc_nic.NIC: one caption from ``members`` = G scans of the same image (repeated trials, or the subjects of
    lc_nic.NIC(n_subjects=G)).  At every token the members' next-word distributions are combined on the device
    (tnt_consensus_mix_f32, include/tnt_hip.h) and the common word is fed back to all of them.
      members  G, 1 .. 16.  The decode inputs hold G * M rows, member-major: rows [g*M, (g+1)*M) are member g's scans of the
               M images (np.concatenate([trial1, trial2, ...])); start_seq has M entries
      mode     "mean": the weighted mean of the members' softmaxes (the standard captioning ensemble);
               "logmean": the renormalised weighted geometric mean
      weights  G finite numbers > 0, normalised here to sum 1; None: 1/G each
    Bad values raise ValueError here, before any launch; what depends on the model or the call is checked by the decode.
    greedy_predict: per token one tnt_consensus_mix_f32 launch takes the place of softmax + argmax, and the mixture's
    first maximum is fed to all members.  sample_predict: the draw is from the mixture (row m on the Philox stream row m
    of a plain decode of M scans uses), and one tnt_consensus_spread_i32 launch carries it to the members.  beam_search:
    the beams of image m are scored by the mixture of its G scans.  The decoder rows are [G][M][k]; the mix launch takes
    the softmax's place, the expansion runs on the M * k mixed rows, one spread launch carries token, parent and finished
    flag to the member rows, and every member's state is gathered by its spread parents.  What a decode returns per
    caption (words, probabilities: the mixtures, sequences, scores) has M rows.  None: the decode as it is without the
    keyword.
    One model object decodes all members: mixing several models is out of scope (the row layout leaves room for it), and
    so are NICfc, the ThinkAndTell / ShowAndTell generators and score_captions."""

    MAX_MEMBERS = 16
    MODES = ("mean", "logmean")

    def __init__(self, members, mode="mean", weights=None):
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or not 1 <= members <= self.MAX_MEMBERS:
            raise ValueError(f"members must be an int in [1, {self.MAX_MEMBERS}], got {members!r}")
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {self.MODES}, got {mode!r}")
        if weights is not None:
            try:
                w = np.asarray(list(weights), dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError(f"weights must be {int(members)} numbers > 0 or None, got {weights!r}") from None
            if w.shape[0] != members or not np.all(np.isfinite(w)) or not np.all(w > 0):
                raise ValueError(f"weights must be {int(members)} finite numbers > 0 or None, got {weights!r}")
            w = (w / w.sum()).astype(np.float32)
            if not np.all(w > 0):
                raise ValueError(f"weights must stay > 0 in float32 once normalised, got {weights!r}")
            weights = tuple(float(v) for v in w)
        self.members, self.mode, self.weights = int(members), mode, weights

    def __repr__(self):
        return f"Consensus(members={self.members}, mode={self.mode!r}, weights={self.weights})"


class _ConsensusDecode:
    """The host part of a consensus decode (ModelBase._consensus) of ``M`` samples x ``k`` beams from G members: the
    decoder runs G*M*k rows (member-major, each member slab laid out [M][k]), the mixture lives on Rm = M*k rows.  Owns
    the device buffers, the per-step launches and the suffix of the capture key."""

    def __init__(self, model, c, M, k=1):
        self._setup(model, c.members, M, k)
        self.mode = Consensus.MODES.index(c.mode)
        self.w = None
        if c.weights is not None:       # one small buffer per distinct weight vector: the vector is part of the capture key
            if ("w", c.weights) not in self._bufs:
                self._bufs["w", c.weights] = torch.tensor(c.weights, dtype=torch.float32).to(model.device)
            self.w = self._bufs["w", c.weights]
        self.key = ("consensus", self.G, c.mode, c.weights)

    def _setup(self, model, G, M, k):
        self.be, self.V, self.ldV, self.G, self.M, self.k = model.be, model.V, model.ldV, G, M, k
        self.Rm, self.rows = M * k, G * M * k
        self._bufs = model._decode_bufs("_cons_bufs")
        self._model = model

    def bufs(self, max_len, steps):
        """static buffers per (G, M, k, max_len): start (rows, 1) int32, the start token of every member row; logits
        (rows, ldV), one step's member logits; mix (steps, Rm, ldV), the
        mixtures (steps = max_len keeps every step's for the return, 1 reuses one slab); pick (max_len, Rm) int32, what the
        sampler chose on the mixed rows; ids / par (max_len, rows) and fin (rows) int32, the choice on the member rows"""
        key = (self.G, self.M, self.k, max_len, steps)
        if key not in self._bufs:
            f, i32 = self._model._f, torch.int32
            self._bufs[key] = dict(start=f(self.rows, 1, dtype=i32), logits=f(self.rows, self.ldV), mix=f(steps, self.Rm, self.ldV),
                                   pick=f(max_len, self.Rm, dtype=i32), ids=f(max_len, self.rows, dtype=i32),
                                   par=f(max_len, self.rows, dtype=i32), fin=f(self.rows, dtype=i32))
        return self._bufs[key]

    def mix(self, logits, mix, token=None):
        """one step: the member rows' logits [rows][ldV] -> the mixture [Rm][ldV]; token (rows,) int32: its argmax, on
        every member row"""
        self.be.consensus_mix(logits, self.ldV, self.V, self.Rm, self.G, self.w, self.mode, mix, self.ldV, token)

    def spread(self, token, parent, fin, token_out, parent_out, fin_out):
        """what the step chose on the mixed rows, carried to the member rows"""
        self.be.consensus_spread(token, parent, fin, self.Rm, self.G, token_out, parent_out, fin_out)


class Guidance:
    """Classifier-free guidance (context-aware / contrastive decoding), for the ``guidance=`` keyword of greedy_predict,
    sample_predict and beam_search of nic.NIC and lc_nic.NIC: at every token the next-word distribution given the scan is
    contrasted on the device with the one the same model gives for a null scan (tnt_guidance_mix_f32, include/tnt_hip.h),
    log p = lc + scale * (lc - ln) renormalised, so that words the scan makes more likely than the language prior does
    are promoted; the common word is fed back to the scan's row and to the null row.
      scale         finite, >= 0; 0 leaves the conditional distribution
      null          the null scan: None, the model's null_scan (the null of its ScanDropout, which it was trained on) or,
                    without one, the all-zero scan (the mean of z-scored betas); an array (N,), one null scan
                    shared by every image; an array (M, N), one per image of the decoded batch
      plausibility  in [0, 1) (0: off): tokens whose conditional probability is below plausibility times the conditional
                    maximum are banned (Li et al. 2022), which keeps a large scale from promoting implausible words
    Bad values raise ValueError here, before any launch; what depends on the model or the call (the shape of ``null``
    against the batch) is checked by the decode.  The decode runs 2 * M decoder rows, the M scans and behind them their
    null scans (a0, c0 repeated), in beam_search [2][M][k].  Per token one tnt_guidance_mix_f32 launch takes the place of
    the softmax (in greedy_predict, of softmax + argmax); the guided distribution's first maximum, or sample_predict's
    draw from it (row b on the Philox stream row b of a plain decode uses), is fed to both rows, and beam_search runs on
    the M * k guided rows exactly as a consensus of two members does (spread, state gather by the spread parents), so its
    scores are sums of guided log-probabilities.  The returned probabilities are the guided distributions.
    ``constraints`` composes (the bans of both rows coincide); consensus, diverse beams and n_subjects > 1 do not.  None
    or a neutral object: the decode as it is without the keyword.  Out of scope: a separately
    trained unconditional model as the null member, guidance with consensus or diverse beams, NICfc, the ThinkAndTell /
    ShowAndTell generators and score_captions."""

    def __init__(self, scale, null=None, plausibility=0.0):
        is_num = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
        f32max = float(np.finfo(np.float32).max)
        if not is_num(scale) or not np.isfinite(scale) or scale < 0 or float(scale) > f32max:
            raise ValueError(f"scale must be a finite number >= 0 (0: off), got {scale!r}")
        if not is_num(plausibility) or not np.isfinite(plausibility) or not 0 <= plausibility < 1 or not np.float32(plausibility) < 1:
            raise ValueError(f"plausibility must be a number in [0, 1) (0: off), got {plausibility!r}")
        if null is not None:
            try:
                v = null.detach().cpu().numpy() if isinstance(null, torch.Tensor) else np.asarray(null)
                v = np.array(v, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"null must be None or an array (N,) or (M, N) of numbers, got {null!r}") from None
            if v.ndim not in (1, 2) or v.size == 0 or not np.all(np.isfinite(v)):
                raise ValueError(f"null must be None or a finite, non-empty array (N,) or (M, N), got shape {v.shape}")
            null = v
        self.scale, self.null, self.plausibility = float(scale), null, float(plausibility)

    @property
    def neutral(self):
        """scale and plausibility are both off (in float32): the decode runs as without guidance"""
        return np.float32(self.scale) == 0 and np.float32(self.plausibility) == 0

    def __repr__(self):
        null = "None" if self.null is None else f"<array {self.null.shape}>"
        return f"Guidance(scale={self.scale}, null={null}, plausibility={self.plausibility})"


def _check_rate(what, rate):
    """a dropout probability of the input corruption: a finite number in [0, 1] (bool and str refused) -> float"""
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)) or not np.isfinite(rate):
        raise ValueError(f"{what} rate must be a finite number in [0, 1], got {rate!r}")
    if not 0 <= rate <= 1:
        raise ValueError(f"{what} rate must be in [0, 1] (0: off), got {rate!r}")
    return float(rate)


class ScanDropout:
    """Scan dropout, the condition dropout of classifier-free guidance (Ho & Salimans 2022), for the ``scan_dropout=``
    keyword of nic.NIC and lc_nic.NIC: in train_step, with probability ``rate`` per sample, the whole scan row of the staged
    batch is replaced by the null scan (tnt_input_corrupt_f32, include/tnt_hip.h), so the model learns p(caption | null)
    beside p(caption | scan) and ``guidance=Guidance(scale, null=None)`` contrasts against a distribution it was trained on.
      rate   a finite number in [0, 1]; 0 is the model without the option
      null   the null scan: None, the all-zero scan; an array (N,) of finite numbers, checked against the model's input
             width by the model.  ``model.null_scan`` returns it, and a guided decode with null=None takes it from there
    Row b of step s fires when the 24-bit uniform of element b of the Philox stream (seed, S_SCAN_DROP, s) is below the
    rate.  Bad values raise ValueError here, before any launch.  test_step, __call__, the decodes and score_captions never
    corrupt their input."""

    def __init__(self, rate, null=None):
        self.rate = _check_rate("scan dropout", rate)
        if null is not None:
            try:
                v = null.detach().cpu().numpy() if isinstance(null, torch.Tensor) else np.asarray(null)
                v = np.array(v, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"null must be None or an array (N,) of numbers, got {null!r}") from None
            if v.ndim != 1 or v.size == 0 or not np.all(np.isfinite(v)):
                raise ValueError(f"null must be None or a finite, non-empty array (N,), got shape {v.shape}")
            null = v
        self.null = null

    @property
    def neutral(self):
        """the rate is 0 in float32: the step runs as without the option"""
        return np.float32(self.rate) == 0

    def __repr__(self):
        null = "None" if self.null is None else f"<array {self.null.shape}>"
        return f"ScanDropout(rate={self.rate!r}, null={null})"


class WordDropout:
    """Word dropout (Bowman et al. 2016, "Generating sentences from a continuous space"), for the ``word_dropout=`` keyword
    of nic.NIC and lc_nic.NIC: in train_step, with probability ``rate`` per fed caption token, the token is replaced by the
    unknown-word id ``unk_id`` (tnt_input_corrupt_f32, include/tnt_hip.h); the targets stay, so the decoder cannot lean on
    the previous words alone and has to read the scan.  Column 0 (the start token) and id 0 (padding, the mask id) are never
    replaced.
      rate    a finite number in [0, 1]; 0 is the model without the option
      unk_id  an int >= 1; the model checks it against its vocabulary size
    Position (b, t) of step s fires when the 24-bit uniform of element b * T + t of the Philox stream (seed, S_WORD_DROP, s)
    is below the rate.  Bad values raise ValueError here, before any launch."""

    def __init__(self, rate, unk_id):
        self.rate = _check_rate("word dropout", rate)
        if isinstance(unk_id, bool) or not isinstance(unk_id, (int, np.integer)) or unk_id < 1:
            raise ValueError(f"unk_id must be an int >= 1 (0 is the padding id), got {unk_id!r}")
        self.unk_id = int(unk_id)

    @property
    def neutral(self):
        """the rate is 0 in float32: the step runs as without the option"""
        return np.float32(self.rate) == 0

    def __repr__(self):
        return f"WordDropout(rate={self.rate!r}, unk_id={self.unk_id})"


class _GuidanceDecode(_ConsensusDecode):
    """The host part of a guided decode (ModelBase._guidance) of ``M`` samples x ``k`` beams: the consensus helper with the
    two members (scan, null scan) and tnt_guidance_mix_f32 as the mix launch; buffers and spread are inherited."""

    def __init__(self, model, g, M, k=1):
        self._setup(model, 2, M, k)
        self.scale, self.plaus = float(np.float32(g.scale)), float(np.float32(g.plausibility))
        self.key = ("guidance", self.scale, self.plaus)

    def mix(self, logits, mix, token=None):
        """one step: the 2 * Rm member rows' logits [rows][ldV] -> the guided distribution [Rm][ldV]; token (rows,) int32:
        its argmax, on both member rows"""
        self.be.guidance_mix(logits, self.ldV, self.V, self.Rm, self.scale, self.plaus, mix, self.ldV, token)


def check_sampling(top_k, top_p, temperature):
    """host validation of the sampling filters (tnt_sample_topkp_f32): top_k an int >= 0 (0 = off), 0 < top_p <= 1
    (1 = off), temperature > 0.  Returns (int top_k, float top_p, float temperature); ValueError otherwise."""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0:
        raise ValueError(f"top_k must be an int >= 0 (0: no top-k filter), got {top_k!r}")
    try:
        p, t = float(top_p), float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"top_p and temperature must be numbers, got {top_p!r}, {temperature!r}") from None
    if not 0.0 < p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1] (1: no nucleus filter), got {top_p!r}")
    if not t > 0.0:
        raise ValueError(f"temperature must be > 0, got {temperature!r}")
    return int(top_k), p, t


def check_length_penalty(length_penalty):
    """host validation of beam search's length_penalty: a finite number >= 0.  Returns it as a float; ValueError
    otherwise."""
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float, np.integer, np.floating)):
        raise ValueError(f"length_penalty must be a finite number >= 0, got {length_penalty!r}")
    lp = float(length_penalty)
    if not (np.isfinite(lp) and lp >= 0.0):
        raise ValueError(f"length_penalty must be a finite number >= 0, got {length_penalty!r}")
    return lp


def check_beam(beam_width, max_len, end_id, length_penalty, V):
    """host validation of beam search's arguments: beam_width an int in [1, 16] (tnt_beam_step_f32's limit), max_len an
    int >= 1, end_id an int in [-1, V) (-1: never ends), length_penalty as check_length_penalty.  Returns
    (beam_width, max_len, end_id, length_penalty); ValueError otherwise."""
    def is_int(x):
        return not isinstance(x, bool) and isinstance(x, (int, np.integer))
    if not is_int(beam_width) or not 1 <= beam_width <= 16:
        raise ValueError(f"beam_width must be an int in [1, 16], got {beam_width!r}")
    if not is_int(max_len) or max_len < 1:
        raise ValueError(f"max_len must be an int >= 1, got {max_len!r}")
    if not is_int(end_id) or not -1 <= end_id < V:
        raise ValueError(f"end_id must be an int in [-1, {V}) (-1: no end token), got {end_id!r}")
    return int(beam_width), int(max_len), int(end_id), check_length_penalty(length_penalty)


class BeamDiversity:
    """Diverse (group) beam search with Hamming diversity (Vijayakumar et al. 2016/2018), for the ``diversity=`` keyword
    of beam_search of nic.NIC and lc_nic.NIC.  The definition is tnt_beam_step_diverse_f32's (include/tnt_hip.h):
      groups   Gd >= 1; it must divide beam_width.  The k beams of a sample search as Gd groups of k' = k / Gd beams; at
               every token the groups choose one after the other
      penalty  lambda, finite and >= 0: a candidate's selection key is its score minus lambda times the number of beams the
               earlier groups of the sample chose at this token with the same word.  The carried scores stay sums of
               log-probabilities: the penalty steers the selection only
    groups = 1 is plain beam search, whatever the penalty; penalty = 0 gives Gd equal groups.  Bad values raise ValueError
    here, before any launch; that groups divides the beam width is checked by the search.
    One tnt_beam_step_diverse_f32 launch takes the expansion's place (with consensus too, on the M * k mixed rows), and
    every group starts from its own copy of the start state.  The results are group-major: group g's k' results sit best
    first at slots g*k' .. g*k' + k' - 1 (the group index of the k slots is np.repeat(np.arange(Gd), k')), group 0 is the
    plain search of width k', and ``length_penalty`` reorders within a group only.  ``constraints`` composes unchanged.
    None or groups = 1: the search as it is without the keyword."""

    def __init__(self, groups, penalty=0.5):
        if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or groups < 1:
            raise ValueError(f"groups must be an int >= 1, got {groups!r}")
        lam = penalty
        if (isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not np.isfinite(lam)
                or lam < 0 or float(lam) > float(np.finfo(np.float32).max)):
            raise ValueError(f"penalty must be a finite number >= 0, got {lam!r}")
        self.groups, self.penalty = int(groups), float(np.float32(lam))

    def __repr__(self):
        return f"BeamDiversity(groups={self.groups}, penalty={self.penalty})"


def check_diversity(diversity, beam_width):
    """host validation of beam search's ``diversity=``: None or a BeamDiversity whose groups divide beam_width.  Returns
    (groups, penalty), or None for plain beam search (None, or one group); ValueError otherwise."""
    if diversity is None:
        return None
    if not isinstance(diversity, BeamDiversity):
        raise ValueError(f"diversity must be a model_base.BeamDiversity or None, got {diversity!r}")
    if beam_width % diversity.groups != 0:
        raise ValueError(f"beam_width {beam_width} is not a multiple of the {diversity.groups} groups of {diversity!r}")
    return (diversity.groups, diversity.penalty) if diversity.groups > 1 else None


def beam_init_scores(M, k, groups=1):
    """beam search's scores in front of step 0, float32 (M * k,): the k' = k / groups beams of every group of a sample are
    copies of the start state, so only the group's first counts (0) and the others cannot win (-1e30).  groups = 1 is the
    plain search's rule: only beam 0 of the sample counts."""
    init = np.full((M, groups, k // groups), -1e30, np.float32)
    init[:, :, 0] = 0.0
    return init.reshape(M * k)


def beam_backtrack(parents, tokens, M, k):
    """the paths of beam search's M * k final beams from the (max_len, M * k) parent rows and tokens of every step (host
    arrays): walks the parent links of every beam at once, last step first.  Returns (M, k, max_len) int64."""
    max_len = len(tokens)
    seqs = np.zeros((max_len, M * k), np.int64)
    row = np.arange(M * k)
    for i in range(max_len - 1, -1, -1):
        seqs[i] = tokens[i, row]
        row = parents[i, row]
    return seqs.T.reshape(M, k, max_len)


def length_normalise(seqs, scores, end_id, length_penalty, groups=1):
    """Length normalisation of beam search's k finished results per sample (seqs (B, k, max_len), scores (B, k), best
    first): the results are reordered by the key  score / ((5 + L) / 6) ** length_penalty, computed in float64, where L
    is the number of tokens up to and including the first end_id (max_len if there is none).  Ties keep the search's
    rank order.  Returns (seqs, key as float32).  length_penalty = 0: the key is the raw sum, the order unchanged.
    ``groups`` > 1 (diverse beam search's group-major results): every group of k / groups results is reordered on its
    own and stays at its slots."""
    seqs = np.asarray(seqs)
    B, k, T = seqs.shape
    if groups > 1:
        s, key = length_normalise(seqs.reshape(B * groups, k // groups, T), np.asarray(scores).reshape(B * groups, -1),
                                  end_id, length_penalty)
        return s.reshape(B, k, T), key.reshape(B, k)
    hit = seqs == end_id
    L = np.where(hit.any(axis=2), hit.argmax(axis=2) + 1, T)
    key = np.asarray(scores, np.float32).astype(np.float64) / ((5.0 + L) / 6.0) ** float(length_penalty)
    order = np.argsort(-key, axis=1, kind="stable")
    return (np.take_along_axis(seqs, order[:, :, None], axis=1),
            np.take_along_axis(key, order, axis=1).astype(np.float32))


class _TokenChoice:
    """The per-token choice of a greedy or sampled decode over ``rows`` decoder rows (ModelBase._decode_setup's B), from
    the head GEMM's logits to the token that is fed back.  ``mode``: None, the first maximum; (temperature, sample_step),
    the unfiltered draw (tnt_sample_rows_f32: the stream step is a launch argument, so this decode cannot be captured);
    (temperature, top_k, top_p, sample_step), the filtered draw (tnt_sample_topkp_f32: the step reaches a replay through
    the model's step word).  ``con`` / ``cons``: the constraint and member helpers, or None.  Static buffers per (rows,
    max_len), the member helper's own with one: start (rows, 1) int32, the start tokens; probs (max_len, M, ldV), every
    step's distributions (with a member helper the mixtures); ids (max_len, rows) int32, the word chosen on every row."""

    def __init__(self, model, rows, max_len, mode, con, cons):
        be, V, ldV, seed = model.be, model.V, model.ldV, model.seed
        self.be, self.V, self.ldV, self.rows, self.con, self.cons = be, V, ldV, rows, con, cons
        if cons is not None:                           # the mixtures are M rows per step, not rows
            cb = cons.bufs(max_len, max_len)
            self.start, self.probs, self.ids = cb["start"], cb["mix"], cb["ids"]
            self.pick, self.member_logits = cb["pick"], cb["logits"]
        else:
            bufs = model._dec_bufs
            if (rows, max_len) not in bufs:
                f, i32 = model._f, torch.int32
                bufs[rows, max_len] = (f(rows, 1, dtype=i32), f(max_len, rows, ldV), f(max_len, rows, dtype=i32))
            self.start, self.probs, self.ids = bufs[rows, max_len]
        self.draw = None                               # draw(p, out, n, i): token i of the n rows of p
        if mode is not None and len(mode) == 4:
            step_word = model._sample_step_word(mode[3])
            self.draw = lambda p, out, n, i: be.sample_topkp(p, out, n, V, ldV, mode[0], mode[1], mode[2], False, seed,
                                                             S_SAMPLE + i, 0, step_word)
        elif mode is not None:
            self.draw = lambda p, out, n, i: be.sample_rows(p, out, n, V, ldV, mode[0], False, seed, S_SAMPLE + i, mode[1])

    def logits(self, i):
        """where the head GEMM of step i writes: the step's row of probs (softmax in place), or the member rows' slab"""
        return self.probs[i] if self.cons is None else self.member_logits

    def step(self, i, logits, prev):
        """decode step i: constrain, then softmax + argmax or draw, or with a member helper the mix (+ argmax inside the
        launch, or draw on the mixed rows + spread).  ``prev`` (rows, 1): the tokens step i was fed.  Returns the tokens
        to feed step i + 1, ids[i] as (rows, 1)."""
        be, cons, ids = self.be, self.cons, self.ids[i]
        if self.con is not None:
            self.con.step(i, logits, self.ldV, prev if i > 0 else None)
        if cons is None:
            be.softmax_cce(logits, None, logits, None, None, None, self.rows, self.V, self.ldV, 0.0)
            if self.draw is None:
                be.argmax_rows(logits, ids, self.rows, self.V, self.ldV)
            else:
                self.draw(logits, ids, self.rows, i)
        elif self.draw is None:
            cons.mix(logits, self.probs[i], ids)
        else:               # row r draws from the stream row r of a plain decode draws from; the choice goes to every member
            cons.mix(logits, self.probs[i])
            self.draw(self.probs[i], self.pick[i], cons.Rm, i)
            cons.spread(self.pick[i], None, None, ids, None, None)
        return ids.view(self.rows, 1)


class _BeamDecode:
    """The bookkeeping of a beam search of ``M`` captions x ``k`` beams: scores and finished flags (ping-pong), every
    step's parents and tokens, the step from the head GEMM's logits to the tokens and parent rows the decoder continues
    from, and the finish on the host.  ``expand(p, score_in, fin_in, score_out, parent, token, fin_out)``: the model's
    expansion launch on the M * k rows of p.  ``con`` / ``cons`` / ``div``: what ModelBase._decode_setup returned.
    ``bufs``: the dict the model keeps its static buffers of this search in (score, fin, pt and the initial scores are
    added to it), or None for buffers of this call alone."""

    def __init__(self, model, M, k, max_len, end_id, expand, con, cons, div, bufs=None):
        self.be, self.V, self.ldV, self.M, self.k, self.max_len, self.end_id = model.be, model.V, model.ldV, M, k, max_len, end_id
        self.expand, self.con, self.cons, self.mix = expand, con, cons, None
        self.Gd = div[0] if div is not None else 1
        bufs = {} if bufs is None else bufs
        if "score" not in bufs:
            f, i32 = model._f, torch.int32
            bufs.update(score=f(2, M * k), fin=f(2, M * k, dtype=i32), pt=f(2, max_len, M * k, dtype=i32))
        init = "init" if div is None else ("init", self.Gd)
        if init not in bufs:                           # step 0: only the first beam of the sample, or of every group, counts
            bufs[init] = torch.from_numpy(beam_init_scores(M, k, self.Gd)).to(model.device)
        self.score, self.fin, self.pt = bufs["score"], bufs["fin"], bufs["pt"]
        self.parents, self.tokens = self.pt[0], self.pt[1]
        self.score[0].copy_(bufs[init])
        self.fin[0].zero_()
        # what the decoder rows read back: the expansion's own outputs or, with a member helper, their spread to the member rows
        self.rows = M * k
        self.tok_d, self.par_d, self.fin_d = self.tokens, self.parents, self.fin
        if cons is not None:
            cb = cons.bufs(max_len, 1)
            self.rows = cons.rows
            self.mix, self.tok_d, self.par_d, self.fin_d = cb["mix"][0], cb["ids"], cb["par"], (cb["fin"], cb["fin"])
            cb["fin"].zero_()

    def step(self, i, logits):
        """search step i on the decoder rows' logits: constrain; the softmax in place, or with a member helper the mixture
        in its place; the expansion on the M * k rows; with a member helper its choice spread to the member rows.  Returns
        (tokens, parents) as (rows, 1): what every decoder row is fed next and the row whose state it continues from."""
        cons, score, fin, parents, tokens = self.cons, self.score, self.fin, self.parents, self.tokens
        tok_d, par_d, fin_d = self.tok_d, self.par_d, self.fin_d
        cur, nxt = i & 1, (i & 1) ^ 1
        if self.con is not None:
            self.con.step(i, logits, self.ldV, tok_d[i - 1] if i > 0 else None, par_d[i - 1] if i > 0 else None, fin_d[cur])
        if cons is None:
            self.be.softmax_cce(logits, None, logits, None, None, None, self.rows, self.V, self.ldV, 0.0)
            self.expand(logits, score[cur], fin[cur], score[nxt], parents[i], tokens[i], fin[nxt])
        else:
            cons.mix(logits, self.mix)
            self.expand(self.mix, score[cur], fin[cur], score[nxt], parents[i], tokens[i], fin[nxt])
            cons.spread(tokens[i], parents[i], fin[nxt], tok_d[i], par_d[i], fin_d[nxt])
        return tok_d[i].view(self.rows, 1), par_d[i].view(self.rows, 1)

    def finish(self, length_penalty):
        """the paths back-tracked on the host from one copy of the parents / tokens: (sequences (M, k, max_len) int64,
        scores (M, k) float32), length-normalised with ``length_penalty`` > 0"""
        pt = self.pt.cpu().numpy()
        final = self.score[self.max_len & 1].cpu().numpy().reshape(self.M, self.k)
        seqs = beam_backtrack(pt[0], pt[1], self.M, self.k)
        if length_penalty > 0:
            return length_normalise(seqs, final, self.end_id, length_penalty, self.Gd)
        return seqs, final


def _r4(n):
    return (n + 3) // 4 * 4


def _interleave(w, U, g):
    """keras [.., gU] (g gate blocks) -> kernel layout [.., U, 4], slots g.. zero."""
    out = np.zeros(w.shape[:-1] + (U, 4), w.dtype)
    out[..., :g] = np.moveaxis(w.reshape(*w.shape[:-1], g, U), -2, -1)
    return out


def _deinterleave(w, g):
    """kernel layout [.., U, 4] -> keras [.., gU]."""
    return np.ascontiguousarray(np.moveaxis(w[..., :g], -1, -2)).reshape(*w.shape[:-2], -1)


def interleave_gates(w, U):
    """keras [.., 4U] (i,f,c~,o blocks) -> kernel layout [.., U, 4]."""
    return _interleave(np.asarray(w), U, 4)


def deinterleave_gates(w):
    """kernel layout [.., U, 4] -> keras [.., 4U]."""
    return _deinterleave(np.asarray(w), 4)


def interleave3(w, U):
    """keras [.., 3U] gate blocks (z, r, h) -> interleaved [.., U, 4] with a zero fourth slot."""
    return _interleave(np.asarray(w, np.float32), U, 3)


def deinterleave3(w):
    return _deinterleave(np.asarray(w), 3)


def _layout(name, keras, device):
    """How a variable of keras shape ``keras`` is stored under the shape ``device`` it was added to the arena with:
    ("copy", 0) equal shapes; ("gates", g) g = 3 or 4 gate blocks [.., gU] interleaved as [.., U, 4]; ("pad", 0) the last
    axis zero-padded (the vocabulary axis, V to ldV); ("reshape", 0) the same elements in the same order."""
    keras, device = tuple(keras), tuple(device)
    if keras == device:
        return "copy", 0
    if (len(device) == len(keras) + 1 and device[-1] == 4 and device[:-2] == keras[:-1]
            and keras[-1] in (3 * device[-2], 4 * device[-2])):
        return "gates", keras[-1] // device[-2]
    if len(device) == len(keras) and device[:-1] == keras[:-1] and device[-1] > keras[-1]:
        return "pad", 0
    if int(np.prod(keras)) == int(np.prod(device)):
        return "reshape", 0
    raise ValueError(f"{name}: no device layout takes the keras shape {keras} to the arena shape {device}")


def pack(arr, device_shape, name="?"):
    """keras-layout array -> the float32 array of ``device_shape`` the arena stores (_layout)."""
    arr = np.asarray(arr, dtype=np.float32)
    kind, g = _layout(name, arr.shape, device_shape)
    if kind == "gates":
        return _interleave(arr, device_shape[-2], g)
    if kind == "pad":
        out = np.zeros(tuple(device_shape), np.float32)
        out[..., :arr.shape[-1]] = arr
        return out
    return np.ascontiguousarray(arr).reshape(tuple(device_shape))


def unpack(arr, keras_shape, name="?"):
    """pack's inverse: the stored array -> a fresh array in the keras layout."""
    kind, g = _layout(name, keras_shape, arr.shape)
    if kind == "gates":
        return _deinterleave(arr, g)
    if kind == "pad":
        return arr[..., :keras_shape[-1]].copy()
    return arr.reshape(tuple(keras_shape)).copy()


class _LayerView:
    """What ``model.get_layer(name)`` returns: get_weights/set_weights in keras layouts
    (main.py:161-162 warm-starts 'lstm' and 'time_distributed_softmax' this way)."""

    def __init__(self, model, name, weight_names):
        self.model, self.name, self.weight_names = model, name, weight_names

    def get_weights(self):
        return [self.model.get_weight(f"{self.name}/{w}") for w in self.weight_names]

    def set_weights(self, weights):
        assert len(weights) == len(self.weight_names), "weight list length mismatch"
        for w, arr in zip(self.weight_names, weights):
            self.model.set_weight(f"{self.name}/{w}", arr)

    @property
    def trainable(self):
        """keras's layer.trainable: False when every variable of the layer is frozen.  Assignable: False freezes the
        layer (model.freeze), True puts its frozen variables back at multiplier 1."""
        names = [n for n in self.model._finetune_vars() if n.rsplit("/", 1)[0] == self.name]
        return not self.model._frozen(*names)

    @trainable.setter
    def trainable(self, value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"trainable must be True or False, got {value!r}")
        names = [n for n in self.model._finetune_vars() if n.rsplit("/", 1)[0] == self.name]
        if not names:
            raise ValueError(f"layer {self.name} has no trainable variable")
        if not value:
            self.model.freeze(*names)
        else:
            self.model.set_lr_multipliers({n: 1.0 for n in names if self.model._lr_mul.get(n) == 0.0})


class DeviceGuardError(RuntimeError):
    """A device-side guard tripped (today: the barrier / census guard of the persistent LSTM kernel).  The step that
    carried it left the model state untouched (the optimizer kernels skip on the error word) and the model has already
    fallen back to the per-step kernels, so the caller may simply run the step again -- ``fit`` does."""


class Metrics(dict):
    """train_step/test_step result: values are 0-d device tensors (no host sync until read).  The step's device guard
    word (ModelBase.GUARD slot of ``met``, copied in the same clone as the metrics) rides along: reading the metrics
    raises DeviceGuardError when it is set, so an invalid step cannot go unnoticed -- and costs no extra sync."""
    _guard = _model = _ring = None

    def guarded(self, model, word):
        self._model, self._guard = model, word
        return self

    def as_floats(self):
        out = {k: float(v) for k, v in self.items()}
        if self._ring is not None:        # values are views of a metrics-ring row (ModelBase._met_snapshot): still this step's?
            row, tag = self._ring
            if int(float(row[-1])) != tag:
                raise RuntimeError(f"these metrics were read more than {ModelBase.METRIC_RING} training steps after their step: "
                                   "the ring row has been reused (read metrics earlier, or set model.metric_ring = False)")
        if self._guard is not None and float(self._guard) != 0.0:
            self._model._on_guard_trip(int(float(self._guard)))
        return out


class EncGram(NamedTuple):
    """By-products of nic.NIC's training forward (tnt_dense_fwd_stream_gram_f32) from which the encoder kernel's clip norm
    follows without a pass over its gradient: the arguments of dense_gram_norm under their names there."""
    pre: torch.Tensor
    bias: torch.Tensor
    gx: torch.Tensor
    nsplit: int
    w2: torch.Tensor
    nw2: int


class EncUpdate(NamedTuple):
    """nic.NIC._bwd_enc's hand-off to the fused update: the encoder kernel ``name`` never has its gradient X^T dpre
    written, the update launches form it from ``x`` [rows][ldx] and ``dpre`` [rows][E] themselves."""
    name: str
    x: torch.Tensor
    dpre: torch.Tensor
    rows: int
    N: int
    E: int
    ldx: int
    gram: Optional[EncGram] = None


class StepTail:
    """What the launches of a fused step leave to its update (ModelBase._update_fused) instead of issuing a launch of their
    own.  ``deferring`` is on inside ModelBase._deferring(); the producers read it and set the fields, which are named
    after the finalize_desc / step_finalize keywords they become (None: not handed over)."""
    FINALIZE = ("x0", "out0", "x1", "out1", "n", "scale",           # the loss / accuracy totals (ModelBase._sum2)
                "x2", "out2", "n2", "scale2",                       # the attention metric's total (lc_nic.NIC._loss_metrics)
                "extra_part", "extra", "n_extra",                   # the sparse Embedding backward's norm partials ...
                "ids_src", "ids_dst", "n_ids")                      # ... and this step's ids, handed on as prev_ids

    def __init__(self, deferring=False):
        self.deferring = deferring
        self.metric_parts_ready = False     # lc_nic.NIC: the forward's Dropout launch left the attention metric's partials
        self.enc = None                     # an EncUpdate (nic.NIC._bwd_enc)
        for k in self.FINALIZE:
            setattr(self, k, None)

    def finalize_kw(self):
        """the keywords of the step's finalize work, whichever launch carries it"""
        return {k: getattr(self, k) for k in self.FINALIZE if getattr(self, k) is not None}


@dataclass
class StepRoute:
    """What one method of a forward / backward pass tells a later method of the same pass: which route it took, and which
    of its buffers the later one reads.  StepTail is what the pass leaves to the update; this is what the pass tells
    itself.  Lifetime: ``model._route`` is replaced by an empty record where a batch is staged (_stage_batch, the models'
    _stage_inputs, nic.NIC._stage_scst), so nothing is inherited from a step that failed midway, and nowhere else: not
    between the forward and the backward of a step, nor between the separately recorded segments of a data-parallel step.
    Every field holds its "nothing handed over" value until its producer sets it."""
    # ---- the staging launch -> the step
    head_map_fresh: bool = False    # _stage_batch built the head's row map (compact_head) -> nic.NIC.train_step, _forward,
    #                                 _loss_metrics, _bwd_head, _bwd_seq_lstm: Out, logits and dlogits hold the distinct rows
    stage_fwd_done: bool = False    # _stage_batch ran the encoder forward too (stage_fwd) -> nic.NIC.train_step, _forward
    masks_staged: bool = False      # _stage_batch generated the stored attention keep-masks -> lc_nic.NIC._text_front
    # ---- forward -> backward
    xin_used: Any = None            # nic.NIC._forward: the LSTM input it fed (Xin or Xin_d) -> _bwd_seq_lstm
    hs_used: Any = None             # lc_nic.NIC._forward*: the LSTM output the head read (Hs or Hd) -> _bwd_head
    inter_used: Any = None          # lc_nic.NIC._forward*: what dense_out read (inter or inter_d) -> _bwd_head
    # ---- backward -> backward
    colsum_deferred: Any = None     # nic.NIC._bwd_head: the head-bias column sums' arguments, not issued -> _bwd_seq_lstm
    dxin_done: bool = False         # nic.NIC._bwd_seq_lstm: its pair launch formed dXin -> _bwd_seq_front
    dout_masked: bool = True        # lc_nic.NIC._bwd_head applied the LSTM-output Dropout' to dHs (False: it rides in the
    #                                 backward chain) -> _bwd_chain
    dtext_done: bool = False        # lc_nic.NIC._bwd_chain: its pair launch formed dtext -> _bwd_emb
    dw2_done: bool = False          # lc_nic.NIC._bwd_chain: its second pair launch formed the W2 gradient -> _bwd_front
    emb_rows: Any = None            # the models' Embedding backward: (row gradients [n][E], n, E, ld, arena name) -> _apply_agc


class ModelBase:
    # ---- A/B switches: class attributes, set on a model (``model.name = value``) before its first step.  Each is declared
    # here once with its default; the comment names the other arm and who sets it.  Tools that take switch names from their
    # command line refuse a name no model class declares (tools/switches.py).
    use_gemm3 = True            # False: vendor-library routing (hipBLASLt head, rocBLAS LSTM products); INTEGRATION.md 4, tools/probe/dp_w1_diff.py
    g3_riders = True            # False: bias sums and paired products as launches of their own; tools/probe/dp_w1_diff.py
    g3_force = None             # {(M, N, K, tA, tB, batch): (tile, splitk)}: a gemm3 plan forced per shape; tools/pair_scan.py, tests
    g3_live_map = True          # False: a split product under a live row count keeps the grid map of its full shape, and its pair the two independent plans; tools/ab_attr.py
    g3_min_flops = 3e7          # products below it keep the tiled split-K kernel; tests/test_gpu_compact_head.py
    use_blas = True             # False (with use_gemm3 = False): the round-1 hand-written kernels; INTEGRATION.md 4
    lt_min_flops = 1e9          # hipBLASLt takes the vocabulary-sized products above it (use_gemm3 = False); tools/lt_tune.py
    use_side_streams = False    # True: independent gradient GEMMs on side streams (measured slower); tools/side_bench.py
    fused_update = True         # False: the unfused step tail (sum2, seg_sqnorm, step_tick, adam); INTEGRATION.md 4, tools/ab_attr.py
    fused_finalize = True       # False: the scalar tail as its own launch (step_finalize); INTEGRATION.md 4, tools/step_breakdown.py
    fused_bn_drop = True        # False: the Dropout / LeakyReLU' beside a BatchNorm as launches of their own; tests/dev_grad_margin.py
    sparse_emb_bwd = True       # False: the dense Embedding backward (and a hipGraph, not a launch plan); INTEGRATION.md 4
    plan_step = True            # False: the single-process step replays as a hipGraph; tools/probe/plan_bench.py
    metric_ring = True          # False: a clone of the metrics buffer behind every step; INTEGRATION.md 4, bench.py
    sync_bn = False             # True: BatchNorm statistics over the global batch; dp.attach(sync_bn=True)
    use_seq_lstm = True         # False: the per-step LSTM kernels; INTEGRATION.md 4, disable_seq_lstm()
    skip_frozen_work = True     # False: the gradient launches of frozen variables run as ever (the table alone freezes); tests/test_host_finetune.py

    # the static buffers of _ConstrainedDecode, of _ConsensusDecode / _GuidanceDecode and of mbr_decode: a dict on the instance
    # from the first such decode on (_decode_bufs).  Not made in the constructor: the tests tell "this model never ran one"
    # by the instance not having the attribute
    _con_bufs = _cons_bufs = _mbr_bufs = None

    GUARD = 7       # slot of ``met`` that carries the device guard word of the step (see Metrics)
    METRIC_RING = 1024      # rows of the metrics ring: a step's Metrics stay readable for this many further training steps
    SUPPORTS_LABEL_SMOOTHING = True     # False where the step does not go through the compile loss (ThinkAndTell generators)
    SUPPORTS_UNLIKELIHOOD = True        # False where the loss is not the (t, b)-ordered caption head (those, and NICfc)
    UNLIKELIHOOD_MAX_T = 64             # loss positions per caption: one wave holds a caption's prefix
    SUPPORTS_TOKEN_WEIGHTS = True       # class_weight / focal_gamma / normalise: as SUPPORTS_UNLIKELIHOOD
    SUPPORTS_GRAD_ACCUMULATION = False  # gradient_accumulation_steps=: True where train_step runs _train_step_accum (nic.NIC, lc_nic.NIC)
    SUPPORTS_DISTILLATION = False       # CategoricalCrossentropy(distillation=) / set_teacher: True on nic.NIC and lc_nic.NIC
    DISTILL_KL = 5                      # slot of ``met`` that carries the mean of kl_row (``distill_kl``)
    # subclasses fill: self.layers_spec = OrderedDict(layer -> [weight names]),
    # self.keras_shapes = {full name: keras shape}
    def __init__(self, device=None, seed=42, use_graph=True, grad_sync=None):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.seed = int(seed)
        self.use_graph = bool(use_graph)
        self.grad_sync = grad_sync          # callable(model) -> None: data-parallel all-reduce hook (dp.py)
        self.dp_world = int(getattr(grad_sync, "world", 1)) if grad_sync is not None else 1
        self.optimizer = None
        self.loss = None
        self.label_smoothing = 0.0          # of the compile loss (CategoricalCrossentropy(label_smoothing=...))
        self.unlikelihood = 0.0             # of the compile loss (CategoricalCrossentropy(unlikelihood=...))
        self.focal_gamma = 0.0              # of the compile loss (CategoricalCrossentropy(focal_gamma=...))
        self.loss_normalise = "count"       # of the compile loss (CategoricalCrossentropy(normalise=...))
        self.class_weight = None            # host copy of the token weights (compile loss / set_class_weight / fit), or None
        self.cw_dev = None                  # the same V floats on the device: an argument of the weighted head launch
        self.distillation = None            # of the compile loss (CategoricalCrossentropy(distillation=...)); None where neutral
        self.teacher = None                 # the frozen model whose logits a distilled step reads (set_teacher)
        self._teacher_adapt = None          # set_teacher(adapt=): maps the student's batch to the teacher's
        self.kl_row = None                  # the distilled head's kl per loss position (_distill_bufs)
        self._teacher_held = None           # (address, row stride, shape) of teacher.logits in the recorded steps (_distill_bufs)
        self.average = None                 # of the compile optimizer (optimizers.MovingAverage / SWA): an optimizers.Average
        self.seg_wd = None                  # decoupled weight decay (compile optimizer's weight_decay): one float per variable on the device, or None
        self.seg_wd_host = None             # the same table on the host (the encoder's fused update takes its entry as a scalar)
        self.gsq = None                     # global-norm clipping: the one float the update launches read (squared norm of the last step)
        self._gclip_host = None             # the optimizer's global_clipnorm as the recorded launches hold it (_sync_lr)
        self._gsq_filed = False             # a step has written gsq (global_grad_norm)
        self.seg_lrm = None                 # learning-rate multipliers / frozen variables: one float per variable on the device, or None
        self.seg_lrm_host = None            # the same table on the host
        self._lr_mul = {}                   # variable name -> multiplier, the entries that are not 1 (set_lr_multipliers, freeze)
        self._skip_key = None               # the frozen variables whose gradient launches the recorded steps leave out
        self.acc_grad = self.acc_sq = None  # gradient accumulation: the arena-sized accumulator and the Embedding norm's float
        self._accum_host = None             # the optimizer's gradient_accumulation_steps as the recorded launches hold it (_sync_lr)
        self._accum_j = 0                   # micro-steps of the open window that are in the accumulator
        self.lr_schedule = None             # of the compile optimizer (learning_rate=<optimizers.schedules object>)
        self.lr_params = None               # its 16 float64 parameters on the device (tnt_lr_schedule_f32)
        self.agc = None                     # adaptive gradient clipping (enable_agc): (clip_factor, eps), or None
        self.adam_t = None                  # the device counter of applied updates; exists once the optimizer state does
        self._swapped = False               # the weight average sits in the weights (swap_weights)
        self._wd_scalar_segs = set()        # variables whose update takes its decay as a scalar argument (_wd_scalar)
        self._lrm_scalar_segs = set()       # ... and its learning-rate multiplier (_lrm_scalar)
        self._fin_arrive = None             # arrival counters of the update launch that carries the finalize work
        self._fin_descs = {}                # its descriptors (finalize_desc), one per distinct argument set
        self._tail = StepTail()             # what a fused step's launches leave to its update (_deferring, _update_fused)
        self._route = StepRoute()           # what a pass tells itself; replaced where a batch is staged
        self.built = False
        self.stop_training = False
        self._graphs = {}
        self._lr_host = None
        # ---- what the model's constructor or its first build replaces
        self.V = None                       # vocabulary size
        self.S = 1                          # subjects (lc_nic.NIC(n_subjects=...))
        self.xT = None                      # lc_nic.NIC: the voxel-major copy of the staged betas, where its encoder reads one
        self.teacher_forcing = True         # lc_nic.NIC(teacher_forcing=False): the free-running decoder
        self.scheduled_sampling = None      # nic.NIC / lc_nic.NIC(scheduled_sampling=...)
        self.self_critical = None           # nic.NIC(self_critical=...)
        self.attention_coverage = None      # lc_nic.NIC(attention_coverage=...)
        self.init_state = None              # lc_nic.NIC(init_state=...)
        self.semantic = None                # nic.NIC(semantic=...)
        self._scan_dropout = self._word_dropout = None      # nic.NIC / lc_nic.NIC(scan_dropout=..., word_dropout=...)
        self._null_dev = None               # the ScanDropout's null scan on the device (None: the all-zero scan)
        self.met = None                     # the metrics buffer (_build)
        # ---- state that exists only once something has asked for it
        self.opt_m = self.opt_avg = None    # the optimizer's first slot and the weight average (_init_optimizer_state)
        self._seq_lstm = False              # the persistent LSTM chain is in use (_init_seq_lstm)
        self.seq_sync = self.seq_xch = None  # its sync state / error word and the BPTT chain's exchange buffer
        self.met_ring = None                # the metrics ring (_ring_args), with ring_t and _ring_host
        self._last_ring = None              # (row, tag) of the ring row the last step's metrics are views of
        self._ring_keys = set()             # the step keys whose update launch files the metrics in the ring (_run_step)
        self._g3_work = self._g3_sync = None    # gemm3's split-K exchange space and error word (_g3_space)
        self._g3_plans = {}                 # (M, N, K, tA, tB, batch, colsum) -> (tile, splitk)
        self._g3_descs = {}                 # gemm3_pair descriptors, one pair per distinct argument set
        self._skw = {}                      # split-K workspaces of the side branches (gemm_sk(ws=...))
        self._side_streams = {}             # side(i)'s streams
        self._side_used = set()             # ... and the ones join() has to wait for
        self._bn_buf = None                 # synchronised BatchNorm's gather scratch (_bn_scratch)
        self._emb_state = None              # ((B, T, name), prev_ids, norm partials, nparts) of the Embedding backward
        self._agc_tab = None                # arena.AgcTable (_apply_agc)
        self._step_word = None              # the device word a captured sampled decode reads its stream step from
        self._score = None                  # score_captions' buffers (_score_state)
        self._dec_bufs = {}                 # _TokenChoice's static buffers per (rows, max_len)

    # ------------------------------------------------------------------ keras surface
    def compile(self, optimizer=None, loss=None, *metrics, run_eagerly=True, freeze=None, lr_multipliers=None, **kw):
        """model.compile(optimizer, loss_object, run_eagerly=True) -- main.py:134.  ``freeze`` (a list of layer / variable
        names) and ``lr_multipliers`` ({name: multiplier}): the config keys of the same names, applied as model.freeze /
        model.set_lr_multipliers apply them."""
        if freeze is not None and (isinstance(freeze, str) or not isinstance(freeze, (list, tuple))):
            raise ValueError(f"freeze must be a list of layer or variable names, got {freeze!r}")
        if lr_multipliers is not None and not isinstance(lr_multipliers, dict):
            raise ValueError(f"lr_multipliers must be a mapping name -> multiplier, got {lr_multipliers!r}")
        mul = self._resolve_lr_multipliers(dict(lr_multipliers or {}, **{n: 0.0 for n in (freeze or ())}))
        eps, alpha = loss_label_smoothing(loss), loss_unlikelihood(loss)
        gamma, mode = loss_focal_gamma(loss), loss_normalise(loss)
        cw = loss_class_weight(loss, self.V)
        distill = loss_distillation(loss)
        avg = optimizer_average(optimizer)
        lr_mul = self._merged_lr_mul(mul)
        compat.check(self, ("label_smoothing", "unlikelihood", "token_weights", "normalise_weights", "distill_loss",
                            "distillation", "average", "weight_decay", "global_clip", "grad_accum", "finetune"),
                     optimizer=optimizer, label_smoothing=eps, unlikelihood=alpha, focal_gamma=gamma,
                     loss_normalise=mode, class_weight=cw, distillation=distill, average=avg, _lr_mul=lr_mul)
        if distill is not None:
            self._check_teacher(self.teacher)
        self.optimizer = optimizer if optimizer is not None else Adam()
        self._lr_mul = lr_mul
        self.loss = loss
        # Fixed here, not read per step: the head launch sits inside captured graphs, with its smoothing, alpha, gamma and
        # mode as arguments.  The averaging launch sits inside the same plans / graphs, and its settings are launch
        # arguments; so does the schedule's launch (tnt_lr_schedule_f32), whose parameters live in a device buffer of the
        # model's.  A change of any of them drops the recordings
        recorded = (eps, alpha, gamma, mode, avg, optimizer_schedule(self.optimizer), distill)
        if recorded != (self.label_smoothing, self.unlikelihood, self.focal_gamma, self.loss_normalise, self.average,
                        self.lr_schedule, self.distillation):
            self._graphs = {}
        (self.label_smoothing, self.unlikelihood, self.focal_gamma, self.loss_normalise, self.average,
         self.lr_schedule, self.distillation) = recorded
        # ... and so does whether there are token weights; the weights themselves are the contents of a device buffer
        self._store_class_weight(cw)
        if self.built:
            self._init_optimizer_state()

    def _token_weights_on(self, pending=None):
        """whether the head launch is tnt_softmax_cce_weighted_f32 (any non-neutral setting).  ``pending``: the values a
        call is about to store, by attribute name (compat.check)"""
        if not pending:
            return self.class_weight is not None or self.focal_gamma > 0 or self.loss_normalise == "weights"
        g = lambda name: pending[name] if name in pending else getattr(self, name)
        return g("class_weight") is not None or g("focal_gamma") > 0 or g("loss_normalise") == "weights"

    def _store_class_weight(self, cw):
        """cw: None or a float32 array of V weights.  The device buffer is written in place where it exists, so a recorded
        plan or a captured graph that holds its address reads the new weights; only a change between no weights and
        weights changes the launch and drops the recordings."""
        if (cw is None) != (self.class_weight is None):
            self._graphs = {}
        if cw is None:
            self.class_weight, self.cw_dev = None, None
            return
        host = torch.from_numpy(np.ascontiguousarray(cw, dtype=np.float32))
        if self.cw_dev is None:
            self.cw_dev = host.to(self.device)
        else:
            self.cw_dev.copy_(host)
        self.class_weight = np.array(cw, dtype=np.float32)

    def set_class_weight(self, class_weight):
        """Replace the token weights of a compiled model: an array-like of V weights, an ``{id: weight}`` dict (missing ids
        weigh 1) or None.  The next step, a replay of a recorded plan or graph included, uses them."""
        compat.check(self, ("token_weights", "normalise_weights"), class_weight=class_weight)
        self._store_class_weight(None if class_weight is None else check_class_weight(class_weight, self.V))

    # ------------------------------------------------------------------ knowledge distillation (distillation= / set_teacher)
    def _distill_on(self, pending=None):
        """whether the training head launch is tnt_softmax_cce_distill_f32 (a non-neutral descriptor)"""
        return (pending["distillation"] if pending and "distillation" in pending else self.distillation) is not None

    def _check_teacher(self, teacher):
        """what is refused of a teacher: a second model, not a feature of this one (compat holds what the student refuses)"""
        if teacher is None:
            return
        no = lambda what: NotImplementedError(compat.DISTILL_REFUSAL.format(what=what))
        if teacher is self:
            raise no("a model cannot be its own teacher (its logits buffer is the one the student's gradient is written to)")
        if not isinstance(teacher, ModelBase) or not teacher.SUPPORTS_DISTILLATION:
            raise no(f"a {type(teacher).__name__} cannot be a teacher")
        if int(teacher.S) > 1:
            raise no("n_subjects > 1 is not supported on the teacher")
        if getattr(teacher, "use_layer_norm", False):
            raise no("an attention-model teacher with use_layer_norm=True is not supported")
        if not teacher.teacher_forcing:
            raise no("a teacher built with teacher_forcing=False is not supported: the teacher's pass is the teacher-forced one")

    def set_teacher(self, teacher, adapt=None):
        """The frozen model a distilled training step (CategoricalCrossentropy(distillation=...)) takes its second target
        from: a nic.NIC or lc_nic.NIC of either family on the same device, with the same vocabulary size and maximum caption
        length.  In front of every distilled train_step it stages the batch and runs its inference forward (no dropout,
        moving BatchNorm statistics, no loss) as a captured sequence of its own; its weights, optimizer state, moving
        statistics and dropout counters are not touched, and a later change of its weights is seen by the next step.
        That forward is always the teacher-forced one over the caption's own words, also for a teacher that was itself
        trained with scheduled_sampling or self_critical (either is a way to train it, not a part of its inference
        forward); a teacher built with teacher_forcing=False is refused.
        ``adapt(data) -> data`` maps the student's ``((scan, cap, a0, c0), target)`` batch to the teacher's (another scan
        width or state size); without it the batch is passed through, and refused where the teacher cannot stage it.
        ``set_teacher(None)`` detaches.  Either drops the recorded plans and graphs."""
        if teacher is None:
            if adapt is not None:
                raise ValueError("adapt= needs a teacher")
        else:
            compat.check(self, ("distillation",), teacher=teacher)     # what the student refuses, descriptor or not
            self._check_teacher(teacher)
            same = teacher.device.type == self.device.type and (teacher.device.index or 0) == (self.device.index or 0)
            if not same:
                raise ValueError(f"the teacher sits on {teacher.device}, the student on {self.device}: both must share a device")
            if int(teacher.V) != int(self.V):
                raise ValueError(f"the teacher's vocabulary has {teacher.V} words, the student's {self.V}")
            if int(teacher.max_length) != int(self.max_length):
                raise ValueError(f"the teacher's maximum caption length is {teacher.max_length}, the student's {self.max_length}")
            if adapt is not None and not callable(adapt):
                raise ValueError(f"adapt must be a callable data -> data, got {adapt!r}")
        self.teacher, self._teacher_adapt = teacher, adapt
        self._teacher_held = None
        self._graphs = {}

    def _distill_bufs(self, B, T):
        """Behind _teach and outside any capture: kl_row of the staged shape, and the address and row stride of the
        teacher's logits as the student's recordings hold them.  The teacher rebuilds its buffers whenever it is staged at
        another shape (its own test_step or decode at another batch size, a second student) and drops only its own
        recordings; a new kl_row or a moved teacher row drops the student's."""
        if self.kl_row is None or self.kl_row.numel() != T * B:
            self.kl_row = self._f(T * B)
            self._graphs = {}
        t = self.teacher
        held = (t.logits.data_ptr(), int(t.ldV), tuple(t.logits.shape))
        if held != self._teacher_held:
            self._teacher_held = held
            self._graphs = {}

    def _distill_begin(self):
        """In front of a train_step's staging: whether the step is a distilled one, behind its refusals"""
        if not self._distill_on():
            return False
        compat.check(self, ("distillation",))
        self._check_teacher(self.teacher)
        if self.teacher is None:
            raise RuntimeError("the compile loss asks for distillation but the model has no teacher: call set_teacher(model) "
                               "before train_step")
        return True

    def _teach(self, data, B, T):
        """The teacher's part of a distilled step, behind the student's staging and in front of its recorded step: stage
        the (adapted) batch on the teacher and run its teacher-forced inference forward, which leaves teacher.logits
        (T * B rows, t-major: the student's row order) where they are.  The teacher's persistent-chain guard word is
        honoured as _guarded does (one host read): fall back to the per-step kernels and run again."""
        t = self.teacher
        batch = data if self._teacher_adapt is None else self._teacher_adapt(data)
        x, cap, a0, c0 = batch[0][:4]
        if np.shape(x)[-1] != t._input_width() or np.shape(a0)[-1] != t.U or np.shape(c0)[-1] != t.U:
            raise ValueError(f"the teacher stages scans of {t._input_width()} columns and states of {t.U} units, the batch holds "
                             f"{np.shape(x)[-1]} and {np.shape(a0)[-1]}: give set_teacher an adapt= that maps the batch")
        if tuple(np.shape(cap)) != (B, T):
            raise ValueError(f"the teacher's captions have shape {tuple(np.shape(cap))}, the student's {(B, T)}")
        t._stage_batch((x, cap, a0, c0), None, t._input_width())
        run = lambda: t._run_captured(("teach", B, T), lambda: t._forward(B, T, False))
        run()
        if t._guard_word() is not None and float(t.met[t.GUARD]) != 0.0:
            t.disable_seq_lstm()
            run()

    def _distill_metric(self, n):
        """the total of kl_row behind a distilled head launch: in the step-finalize launch's free third slot where the step
        defers its totals and the model has not taken the slot, else a launch of its own"""
        out = self.met[self.DISTILL_KL:self.DISTILL_KL + 1]
        t = self._tail
        if t.deferring and t.x2 is None:
            t.x2, t.out2, t.n2, t.scale2 = self.kl_row, out, n, 1.0 / n
        else:
            self.be.sum(self.kl_row, out, n, 1.0 / n)

    def _head_gscale(self, n):
        """The gradient scale of a training head launch over ``n`` loss positions: 1 / n for the mean over the batch,
        divided by the data-parallel world size (the all-reduce is a SUM) and, inside an accumulation window, by its k
        micro-steps (tnt_grad_accumulate_f32 sums them): either sum is then the mean over the global batch."""
        return 1.0 / (n * self.dp_world * (self._accum_host or 1))

    def _head_loss(self, B, T, want_grad):
        """The head launch of _loss_metrics over the T * B position-ordered rows, chosen by the compile loss: label
        smoothing, unlikelihood, token weights / the focal factor / normalise="weights", or the plain softmax-CCE.  Each in
        its training form (dlogits in place, scaled for the mean over the global batch) or its evaluation form
        (probabilities in place, gscale 0): the same objective in both -- keras smooths the evaluation loss too.
        Distillation is a training objective only: its launch exists in the training form, and the evaluation form of a
        distilling model is the plain one."""
        be, n = self.be, T * B
        probs, dlogits = (None, self.logits) if want_grad else (self.logits, None)
        gscale = self._head_gscale(n) if want_grad else 0.0
        if self.label_smoothing > 0:
            be.softmax_cce_smooth(self.logits, self.tgt, probs, self.loss_row, self.corr_row, dlogits, n, self.V, self.ldV,
                                  gscale, self.label_smoothing)
        elif self.unlikelihood > 0:
            # _stage_batch has refused a caption that is too long before any launch of the step
            assert T <= self.UNLIKELIHOOD_MAX_T
            be.softmax_cce_unlikely(self.logits, self.tgt, probs, self.loss_row, self.corr_row, dlogits, B, T, self.V,
                                    self.ldV, gscale, self.unlikelihood)
        elif self._token_weights_on():
            be.softmax_cce_weighted(self.logits, self.tgt, self.cw_dev, probs, self.loss_row, self.corr_row, dlogits, n,
                                    self.V, self.ldV, gscale, self.focal_gamma, self.loss_normalise == "weights")
        elif want_grad and self._distill_on():
            # the training form only: test_step reports the plain cross-entropy.  train_step ran the teacher (_teach)
            d, t = self.distillation, self.teacher
            be.softmax_cce_distill(self.logits, t.logits, self.tgt, self.loss_row, self.kl_row, self.corr_row, dlogits, n,
                                   self.V, self.ldV, t.ldV, gscale, d.alpha, d.temperature)
        else:
            be.softmax_cce(self.logits, self.tgt, probs, self.loss_row, self.corr_row, dlogits, n, self.V, self.ldV, gscale)

    @property
    def be(self):
        return ops.backend()

    def _f(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def _init_optimizer_state(self):
        a = self.arena
        # decoupled weight decay: the per-variable table from the descriptor and its exclusions, which are final from here
        # on (keras: exclude_from_weight_decay raises once the optimizer is built)
        tab = weight_decay_table(self.optimizer, list(a.entries))
        compat.check(self, ("weight_decay", "global_clip", "grad_accum", "finetune"), weight_decay=tab is not None)
        self.opt_m = torch.zeros_like(a.theta)
        self.opt_v = torch.zeros_like(a.theta) if self.optimizer.kind == "adam" else None
        self.adam_t = torch.zeros(1, dtype=torch.int64, device=self.device)
        sched = self.lr_schedule
        # with a schedule the host never writes lr_dev again: every step's tnt_lr_schedule_f32 launch does, from adam_t
        self.lr_dev = torch.tensor([self.optimizer.lr if sched is None else sched(0)], dtype=torch.float32, device=self.device)
        self.lr_t_dev = self._f(1)
        self._lr_host = self.optimizer.lr if sched is None else None
        self._set_lr_schedule(sched)
        # the weight average (optimizers.MovingAverage / SWA): one more slot over the whole arena, padding included (zero in
        # both buffers, and it stays zero).  The first averaging launch overwrites it with the parameters after update
        # max(start_step, 1); until then it holds the initial ones
        self.opt_avg = a.theta.clone() if self.average is not None else None
        self._swapped = False
        self.seg_wd = self.seg_wd_host = None
        self._store_seg_wd(tab)
        getattr(self.optimizer, "_optimizer", self.optimizer)._wd_built = True
        # global-norm clipping: the word tnt_global_sqnorm_f32 writes and every update launch of the step reads
        self.gsq = self._f(1)
        # learning-rate multipliers and frozen variables: the table of what set_lr_multipliers / freeze have asked for so far
        self.seg_lrm = self.seg_lrm_host = None
        self._store_seg_lrm()
        self._gsq_filed = False
        self._gclip_host = self._gclip()
        # gradient accumulation: one more arena-sized buffer and the float beside it, only for a model that accumulates
        self._accum_host = self._accum_k()
        self._accum_j = 0
        self.acc_grad = torch.zeros_like(a.grad) if self._accum_host is not None else None
        self.acc_sq = self._f(1) if self._accum_host is not None else None
        self._graphs = {}

    # ------------------------------------------------------------------ decoupled weight decay (Adam / SGD weight_decay=, AdamW)
    def _store_seg_wd(self, tab):
        """tab: None (nothing decays: the plain update launches) or one decay per variable.  The device table is written in
        place where it exists, so a recorded plan or a captured graph that holds its address decays by the new values; a
        change between no decay and decay changes the launches and drops the recordings, and so does a new value for a
        variable whose update takes its decay as a scalar argument (the encoder's fused update)."""
        if tab is not None and not any(tab):
            tab = None
        old = self.seg_wd_host
        if (tab is None) != (old is None):
            self._graphs = {}
        if tab is None:
            self.seg_wd = self.seg_wd_host = None
            return
        host = np.asarray(tab, dtype=np.float32)
        if old is not None and any(host[s] != old[s] for s in self._wd_scalar_segs):
            self._graphs = {}
        if self.seg_wd is None:
            self.seg_wd = torch.from_numpy(host.copy()).to(self.device)
        else:
            self.seg_wd.copy_(torch.from_numpy(host))
        self.seg_wd_host = host

    def set_weight_decay(self, value):
        """Replace the decay of a compiled and built model: every variable that exclude_from_weight_decay does not name
        decays by ``value`` (a finite float >= 0, or None) from the next step on, a replay of a recorded plan or graph
        included -- the table is a device buffer written in place.  The optimizer descriptor takes the value too."""
        if self.optimizer is None or self.adam_t is None:
            raise RuntimeError("set_weight_decay: compile and build the model first")
        wd = check_weight_decay(value)
        compat.check(self, ("weight_decay",), weight_decay=wd)
        self.optimizer.weight_decay = wd
        self._store_seg_wd(weight_decay_table(self.optimizer, list(self.arena.entries)))

    def _wd_scalar(self, seg):
        """the decay of one variable as the scalar argument of the encoder's fused update"""
        self._wd_scalar_segs.add(seg)
        return float(self.seg_wd_host[seg])

    # ------------------------------------------------------------------ global-norm clipping (Adam / SGD global_clipnorm=)
    def _gclip(self, pending=None):
        """the optimizer's global_clipnorm: a float > 0, or None (off).  ``pending``: as _token_weights_on takes it"""
        opt = pending["optimizer"] if pending and "optimizer" in pending else self.optimizer
        return None if opt is None else check_global_clipnorm(getattr(opt, "global_clipnorm", None))

    def _global_sqnorm(self, fin_kw=None):
        """The reduction launch of a globally clipped step (tnt_global_sqnorm_f32): behind the step's norm launch(es), in
        front of its first update launch and inside the same recorded plan / graph.  ``fin_kw``: the finalize keywords of an
        update that carries the finalize work itself (the fin form, from the span partials); None behind a launch that
        has filed ``sq`` (the table form).  Nothing without global_clipnorm."""
        if self._gclip() is None:
            return
        a = self.arena
        # with a multiplier table: the form that leaves the frozen variables out
        launch = self.be.global_sqnorm if self.seg_lrm is None else \
            (lambda gsq, nseg, **kw: self.be.global_sqnorm_lrmul(gsq, nseg, self.seg_lrm, **kw))
        if fin_kw is None:
            launch(self.gsq, a.nseg, sq_override=a.sq_override, sq=a.sq)
        else:
            extra = {k: fin_kw[k] for k in ("extra_part", "n_extra", "extra_seg") if k in fin_kw}
            launch(self.gsq, a.nseg, sq_override=a.sq_override, partial=a.partial, seg_first=a.spans.seg_first, **extra)
        self._gsq_filed = True

    def global_grad_norm(self):
        """The global gradient norm of the last training step as a float: sqrt of the word its update launches clipped by
        (every variable's gradient with its L2 term, the Embedding by its un-deduplicated rows -- tf.linalg.global_norm).
        A host read.  The number to plot when choosing global_clipnorm; it exists for a model compiled with one."""
        if self.gsq is None or not self._gsq_filed:
            raise RuntimeError("global_grad_norm: no training step with global_clipnorm has run yet")
        return float(self.gsq[0]) ** 0.5

    # ------------------------------------------------------------------ layer freezing and per-variable learning rates (fine-tuning)
    FINETUNE_BATCHNORM = ("freezing a BatchNorm layer ({name}) is not implemented: keras runs a frozen BatchNorm in inference "
                          "mode, on its moving statistics, and the training step here has no such mode.  Freeze the layers "
                          "around it, or give it a small multiplier; LayerNorm gains and biases freeze like any variable")

    def _finetune_vars(self):
        """the names a multiplier can be given to: the variables of the arena, in its order"""
        return list(self.arena.entries)

    def _match_variables(self, name):
        """the variables ``name`` stands for: a layer's (exact layer name), one variable (exact name), else every variable
        whose name contains it -- exclude_from_weight_decay's var_list / var_names rule.  A name that matches nothing raises."""
        if not isinstance(name, str) or not name:
            raise ValueError(f"a layer or variable name must be a non-empty string, got {name!r}")
        names = self._finetune_vars()
        if name in self.layers_spec:
            hit = [n for n in names if n.rsplit("/", 1)[0] == name]
        elif name in names:
            hit = [name]
        else:
            hit = [n for n in names if name in n]
        if not hit:
            raise ValueError(f"{name!r} matches no layer and no trainable variable of {type(self).__name__}; the variables "
                             f"are {names}")
        return hit

    def _resolve_lr_multipliers(self, mapping):
        """{layer / variable name or substring: multiplier} -> {variable name: float}, validated: a finite multiplier
        >= 0, names that match, no frozen BatchNorm.  Later keys override earlier ones where they overlap."""
        out = {}
        for key, mul in mapping.items():
            if isinstance(mul, bool) or not isinstance(mul, (int, float, np.integer, np.floating)) or \
                    not np.isfinite(mul) or mul < 0:
                raise ValueError(f"a learning-rate multiplier must be a finite number >= 0, got {mul!r} for {key!r}")
            for n in self._match_variables(key):
                out[n] = float(np.float32(mul))
        for n, mul in out.items():
            layer = n.rsplit("/", 1)[0]
            # a layer with moving statistics (nic.NIC(norm="layer") keeps the names and normalises per row: no BatchNorm)
            if mul == 0.0 and getattr(self, "norm", "batch") == "batch" and \
                    any(k.startswith(layer + "/moving_") for k in self.keras_shapes):
                raise NotImplementedError(self.FINETUNE_BATCHNORM.format(name=layer))
        return out

    def _merged_lr_mul(self, new):
        return {n: m for n, m in dict(self._lr_mul, **new).items() if m != 1.0}

    def set_lr_multipliers(self, mapping):
        """Per-variable learning-rate multipliers: {layer name, variable name or substring: mul}, mul a finite float >= 0.
        Adam steps the variable by mul * lr_t, SGD by mul * lr, decoupled decay by (mul * lr * wd) * theta, a schedule's rate
        likewise; 1 is the default and restores it, 0 freezes the variable (model.freeze).  Variables not named keep what
        they have.  On a built model the device table is written in place: the next step, a replay of a recorded plan or
        graph included, follows it; only the first multiplier, the last one's removal and a change of which gradient
        launches are left out record the step again."""
        if not isinstance(mapping, dict):
            raise ValueError(f"set_lr_multipliers takes a mapping name -> multiplier, got {mapping!r}")
        new = self._merged_lr_mul(self._resolve_lr_multipliers(mapping))
        compat.check(self, ("finetune",), _lr_mul=new)
        self._lr_mul = new
        if self.adam_t is not None:
            self._store_seg_lrm()

    def freeze(self, *names):
        """Freeze layers or variables (names as set_lr_multipliers takes them): weights and optimizer slots stay
        bit-unchanged by a training step, no decay, no L2 gradient, no share in global_clipnorm's norm; the L2 term stays
        in the reported loss.  adam_t stays global: unfreeze resumes with the old moments at the current step count."""
        self.set_lr_multipliers({n: 0.0 for n in names})

    def unfreeze(self, *names, multiplier=1.0):
        """Back to training, at ``multiplier`` times the learning rate.  A name that matches no frozen variable raises."""
        for n in names:
            if not any(self._lr_mul.get(v) == 0.0 for v in self._match_variables(n)):
                raise ValueError(f"unfreeze: {n!r} matches no frozen variable")
        self.set_lr_multipliers({v: multiplier for n in names for v in self._match_variables(n) if self._lr_mul.get(v) == 0.0})

    def lr_multipliers(self):
        """{variable name: multiplier} of every variable, 1.0 where none was set"""
        return OrderedDict((n, self._lr_mul.get(n, 1.0)) for n in self._finetune_vars())

    def _frozen(self, *names):
        """every one of the variables ``names`` is frozen"""
        return bool(names) and all(self._lr_mul.get(n) == 0.0 for n in names)

    def _skip_grad(self, *names):
        """whether the step leaves out a launch whose only outputs are the gradients of ``names``: all of them frozen
        (skip_frozen_work = False: never -- the table alone freezes them)"""
        return self.skip_frozen_work and self._frozen(*names)

    def _store_seg_lrm(self):
        """The device table from ``_lr_mul``: None while every multiplier is 1 (the plain launches), else one float per
        variable, written in place where the table exists -- a recorded plan or a captured graph that holds its address
        follows.  A change between no table and a table changes the launches and drops the recordings; so does a change of
        the frozen set, which decides the gradient launches a step leaves out (_skip_grad)."""
        entries = self.arena.entries
        tab = None
        if self._lr_mul:
            tab = np.ones(self.arena.nseg, dtype=np.float32)
            for n, mul in self._lr_mul.items():
                tab[entries[n].seg] = mul
        skip = frozenset(n for n, m in self._lr_mul.items() if m == 0.0) if self.skip_frozen_work else frozenset()
        old = self.seg_lrm_host
        if (tab is None) != (old is None) or skip != (self._skip_key or frozenset()):
            self._graphs = {}
        elif tab is not None and any(tab[s] != old[s] for s in self._lrm_scalar_segs):
            self._graphs = {}               # a new scalar argument of the encoder's fused update
        self._skip_key = skip
        if tab is None:
            self.seg_lrm = self.seg_lrm_host = None
            return
        if self.seg_lrm is None:
            self.seg_lrm = torch.from_numpy(tab.copy()).to(self.device)
        else:
            self.seg_lrm.copy_(torch.from_numpy(tab))
        self.seg_lrm_host = tab

    def _lrm_scalar(self, seg):
        """the multiplier of one variable as the scalar argument of the encoder's fused update"""
        self._lrm_scalar_segs.add(seg)
        return float(self.seg_lrm_host[seg])

    def _lrm_kw(self, **decay):
        """the optional trailing arguments of a *_lrmul launch: the global word under global_clipnorm, and ``decay`` where
        the model decays"""
        kw = dict(gsq=self.gsq) if self._gclip() is not None else {}
        if self.seg_wd is not None:
            kw.update(decay)
        return kw

    # ------------------------------------------------------------------ gradient accumulation (Adam / SGD gradient_accumulation_steps=)
    def _accum_k(self, pending=None):
        """the optimizer's gradient_accumulation_steps: an int >= 2, or None (off).  ``pending``: as _token_weights_on
        takes it"""
        opt = pending["optimizer"] if pending and "optimizer" in pending else self.optimizer
        return None if opt is None else check_gradient_accumulation_steps(getattr(opt, "gradient_accumulation_steps", None))

    def _sync_accum(self):
        """In front of every training step (train_step of the accumulating models, in front of the staging; _sync_lr): an
        assignment to optimizer.gradient_accumulation_steps since the state was built.  Allowed between two windows only.
        k scales the head launch's gradient and decides which launches a step is, so the recordings are dropped; so is the
        Embedding backward's state: the dense form and CLOSE leave rows in the gradient table that the sparse form's
        invariant (zero outside the rows of prev_ids) does not allow, and a fresh state starts from a zeroed table."""
        k = self._accum_k()
        if k == self._accum_host or self.adam_t is None:        # (no optimizer state yet: its build reads k)
            return
        if self._accum_j:
            raise RuntimeError(f"gradient_accumulation_steps changed from {self._accum_host} to {k} inside an open window "
                               f"({self._accum_j} micro-steps accumulated): finish the window or call reset_accumulation() "
                               "first")
        compat.check(self, ("grad_accum",))
        self._accum_host = k
        self.acc_grad = torch.zeros_like(self.arena.grad) if k is not None else None
        self.acc_sq = self._f(1) if k is not None else None
        self._graphs = {}
        self._emb_state = None

    @property
    def accumulation_position(self):
        """(j, k): j micro-steps of the current window are in the accumulator, the k-th closes it and applies the update.
        Without accumulation (0, 1): every step is a window of its own.  A host value, no device read."""
        return self._accum_j, self._accum_k() or 1

    def reset_accumulation(self):
        """Drops the open window: the next train_step opens a new one, and what the accumulator holds is never read (OPEN
        overwrites it).  Weights, moments and every counter of applied updates are untouched; the dropout stream has
        advanced by the dropped micro-steps."""
        self._accum_j = 0

    def _train_step_accum(self, B, T, extra=()):
        """One micro-step of an accumulation window (optimizer gradient_accumulation_steps=k), behind the staging; returns
        whether it closed the window, i.e. applied an update.  Accumulation is data parallel in time: the contract of dp.py,
        "G ranks x local batch == one rank on the concatenated batch", with the all-reduce over ranks replaced by a sum
        over micro-steps on the device (tnt_grad_accumulate_f32).  Micro-step j of a window:
          forward + backward, nothing deferred (_train_graph as the generic data-parallel schedule runs it): every gradient
          is written to the arena, the head launch scales dlogits by 1 / (n k) (_head_gscale), the dense Embedding backward
          files its un-deduplicated squared norm, scaled by 1 / k^2, in its sq_override slot;
          j == 0: OPEN (acc = grad);  0 < j < k - 1: ADD (acc += grad);  j == k - 1: CLOSE (grad += acc), then
          _update_graph() unchanged -- norms, L2, global norm, tick, schedule, Adam / SGD with or without decay, averaging.
        With no BatchNorm and no dropout, k micro-steps on consecutive slices of a batch equal one plain step on the whole
        batch up to float32 summation order: the loss mean, every gradient, the per-variable clip norms (sum_j sq_j is the
        Embedding's un-deduplicated norm of the concatenated batch), the global norm, the updated weights.
        Counting -- this library's rule (keras is not at hand to compare its own):
          applied updates: adam_t, model.iterations, the learning-rate schedule, Adam's bias correction, the weight average
          and optimizer.iterations advance on the closing micro-step only;
          micro-steps: drop_step advances on every one (OPEN / ADD tick it, the update's tick does in CLOSE), so every
          micro-batch draws its own masks; BatchNorm's batch statistics are per micro-batch and its moving statistics
          advance per micro-step, as per-replica statistics do under data parallel.
        Micro-batches of different sizes in one window are allowed: the update is the mean of the k micro-batch means, not
        the mean over their samples.  Every micro-step's metrics are its own micro-batch's; L2 is the term of the weights
        its forward used: computed in the opening micro-step (_norms_and_l2, as test_step does), kept in slot 2 of the
        metrics buffer over the window -- the weights do not change inside it -- and recomputed by the closing update.
        A guarded micro-step (the persistent LSTM kernel's error word) leaves accumulator, norm and drop_step alone; the trip
        raises where the metrics are read, and _on_guard_trip reopens the window.
        Each phase is a recording of its own, replayed as a hipGraph: the dense Embedding backward hands its ids on with a
        tensor copy, which a launch plan would drop (see _step_runner)."""
        compat.check(self, ("grad_accum",))
        k, j, a = self._accum_host, self._accum_j, self.arena
        phase = 0 if j == 0 else (2 if j == k - 1 else 1)
        seg = self.emb_seg

        def run():
            with self._deferring(False):
                self._train_graph(B, T)
            if phase == 0:
                self._norms_and_l2(self.met[2:3])
            self.be.grad_accumulate(self.acc_grad, a.grad, a.total, phase, self.acc_sq, a.sq_override[seg:seg + 1],
                                    self.drop_step, guard=self._guard_word())
            if phase == 2:
                self._update_graph()
        self._run_captured(("train_acc", B, T, phase) + tuple(extra), run)
        self._accum_j = 0 if phase == 2 else j + 1
        return phase == 2

    def _sync_lr(self):
        """in front of the update of every training step: the host-set learning rate to the device -- and the refusal of a
        step while the average sits in the weights (swap_weights / averaged_weights)"""
        if self._swapped:
            raise RuntimeError("the averaged weights are swapped in (swap_weights / averaged_weights): a training step would "
                               "train the average and average the raw weights.  Swap back first")
        gclip = self._gclip()
        if gclip != self._gclip_host:
            # optimizer.global_clipnorm was assigned since the state was built: the threshold is an argument of the update
            # launches, and switching it on or off changes which launches run -- the step is recorded again
            compat.check(self, ("global_clip",))
            self._gclip_host = gclip
            self._graphs = {}
        self._sync_accum()      # ... and optimizer.gradient_accumulation_steps, between two windows only
        sched = optimizer_schedule(self.optimizer)
        if sched != self.lr_schedule:
            # optimizer.learning_rate was assigned since compile (a float in place of the schedule, or another schedule):
            # the step's launch sequence changes, so it is recorded again
            self._set_lr_schedule(sched)
            self._lr_host = None
            self._graphs = {}
        if sched is not None:
            return
        if self.optimizer.lr != self._lr_host:
            self.lr_dev.fill_(self.optimizer.lr)
            self._lr_host = self.optimizer.lr

    # ------------------------------------------------------------------ learning-rate schedule (optimizers.schedules)
    def _set_lr_schedule(self, sched):
        """the schedule of the training steps from here on, its 16 float64 parameters in a device buffer of the model's"""
        self.lr_schedule = sched
        self.lr_params = None if sched is None else torch.tensor(sched.params(), dtype=torch.float64, device=self.device)

    def _lr_schedule_launch(self):
        """The schedule's launch of a step (tnt_lr_schedule_f32: lr_dev = schedule(adam_t), adam_t the updates applied so
        far), inside the same recorded plan / graph and in front of the step's first launch that reads lr_dev.  No guard: a
        step whose guard word tripped leaves adam_t, so the next step computes the same value.  Nothing with a float
        learning rate."""
        if self.lr_schedule is not None:
            self.be.lr_schedule(self.adam_t, self.lr_params, self.lr_dev)

    def _lr_metric(self, out):
        """with a schedule: the ``lr`` entry of a training step's metrics is the float32 its update used, read from the
        device with the other metrics (a copy of lr_dev behind the step)"""
        if self.lr_schedule is not None:
            out["lr"] = self.lr_dev.clone()[0]
        return out

    @property
    def iterations(self):
        """keras's optimizer.iterations: the updates applied so far, read from the device counter (a guarded step does not
        count); what the learning-rate schedule, scheduled sampling and the weight average see"""
        return 0 if self.adam_t is None else int(self.adam_t[0])

    def set_iterations(self, n):
        """Writes the update counter, and nothing else (the dropout stream's counter stays): a run continued from
        load_weights with fit(initial_epoch=) puts the learning-rate schedule where it left off.  Adam's bias correction
        reads the same counter."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"iterations must be an int >= 0, got {n!r}")
        if self.adam_t is None:
            raise RuntimeError("set_iterations: the counter exists once the optimizer state does (compile and build the model)")
        self.adam_t.fill_(int(n))

    def _apply_optimizer(self):
        """per-variable clipnorm + Adam/SGD (optimizer.apply_gradients, lc_NIC.py:389).  Its callers have run _norms_and_l2:
        under global_clipnorm the reduction launch reads the table that left."""
        self._global_sqnorm()
        self._tick()
        if self.optimizer.kind == "adam":
            self._adam_update(self._spans())
        else:
            self._sgd_update(self._spans())
        # the tick precedes the update here: adam_t is the number of applied updates when the averaging launch starts
        self._average_update()

    # ---- the update launches, one helper each.  Under decoupled weight decay (``seg_wd`` set) a helper issues the decaying
    # entry point in the plain one's place; its callers pass what differs between them -- the spans, the metrics ring, the
    # finalize descriptor -- and do not know that the decay exists.
    # Under global-norm clipping (``_gclip()`` set) a helper issues the *_gclip entry instead, with the global threshold as its
    # clipnorm, the model's ``gsq`` word and the decay, if any, as its trailing arguments (_gclip_kw).
    def _clip(self):
        """the clip threshold as the launches take it: the optimizer's clipnorm (0 = no clipping), or its global_clipnorm"""
        g = self._gclip()
        if g is not None:
            return g
        clip = self.optimizer.clipnorm
        return clip if clip is not None else 0.0

    def _gclip_kw(self, **decay):
        """the trailing arguments of a *_gclip launch: the global word, and ``decay`` where the model decays"""
        return dict(gsq=self.gsq, **(decay if self.seg_wd is not None else {}))

    def _spans(self, s1=0):
        """(span_seg, span_off, span_len, nspan) of the arena's spans from span ``s1`` on, as the norm and update launches
        take them"""
        sp = self.arena.spans
        return sp.span_seg[s1:], sp.span_off[s1:], sp.span_len[s1:], sp.nspan - s1

    def _adam_update(self, spans, ring=None):
        """clip + Adam over ``spans`` (_spans, or an arena.seg_slice's): tnt_adam_f32 / tnt_adamw_f32.  ``ring``: _ring_args()"""
        be, a, opt = self.be, self.arena, self.optimizer
        seg, off, length, nspan = spans
        args = (a.theta, self.opt_m, self.opt_v, a.grad, seg, off, length, a.seg_l2, a.sq, a.sq_override, nspan, 0.0,
                self.lr_t_dev, opt.beta_1, opt.beta_2, opt.epsilon, self._clip())
        if self.seg_lrm is not None:
            be.adam_lrmul(*args, self.seg_lrm, **self._lrm_kw(lr=self.lr_dev, seg_wd=self.seg_wd), guard=self._guard_word(),
                          **(ring or {}))
        elif self._gclip() is not None:
            be.adam_gclip(*args, **self._gclip_kw(lr=self.lr_dev, seg_wd=self.seg_wd), guard=self._guard_word(), **(ring or {}))
        elif self.seg_wd is None:
            be.adam(*args, guard=self._guard_word(), **(ring or {}))
        else:
            be.adamw(*args, self.lr_dev, self.seg_wd, guard=self._guard_word(), **(ring or {}))

    def _adam_fin_update(self, spans, desc, ring):
        """clip + Adam over ``spans`` with the step's finalize work ``desc`` (finalize_desc) inside the launch:
        tnt_adam_fin_f32 / tnt_adamw_fin_f32.  The descriptor's lr is lr_dev: the decay reads the step's rate through it"""
        be, a, opt = self.be, self.arena, self.optimizer
        seg, off, length, nspan = spans
        args = (a.theta, self.opt_m, self.opt_v, a.grad, seg, off, length, a.sq_override, nspan, opt.epsilon, self._clip(), desc)
        if self.seg_lrm is not None:
            be.adam_fin_lrmul(*args, self.seg_lrm, **self._lrm_kw(seg_wd=self.seg_wd), **ring)
        elif self._gclip() is not None:
            be.adam_fin_gclip(*args, **self._gclip_kw(seg_wd=self.seg_wd), **ring)
        elif self.seg_wd is None:
            be.adam_fin(*args, **ring)
        else:
            be.adamw_fin(*args, self.seg_wd, **ring)

    def _enc_adam_update(self, enc, fin):
        """The encoder kernel's fused update (``enc``: an EncUpdate): clip + Adam on the strips of X^T dpre as they leave
        the MFMAs.  ``fin``: the form that sums the variable's clip norm from its span partials itself
        (tnt_dense_dw_adam_fin_f32 / tnt_dense_dw_adamw_fin_f32), else the one that reads it from ``sq``
        (tnt_dense_dw_adam_f32 / tnt_dense_dw_adamw_f32).  The decaying forms take the variable's decay as a scalar."""
        be, a, sp, opt = self.be, self.arena, self.arena.spans, self.optimizer
        e = a.entries[enc.name]
        sl, one = slice(e.off, e.off + e.size), slice(e.seg, e.seg + 1)
        norm = (a.partial, sp.first_host[e.seg], sp.first_host[e.seg + 1]) if fin else (a.sq[one],)
        args = (enc.x, enc.dpre, a.theta[sl], self.opt_m[sl], self.opt_v[sl], e.l2, *norm, a.sq_override[one], self.lr_t_dev,
                opt.beta_1, opt.beta_2, opt.epsilon, self._clip(), enc.N, enc.E, enc.rows, enc.ldx)
        if self.seg_lrm is not None:
            # the multiplier forms take the variable's multiplier as a scalar, as the decaying forms take its decay
            kw = self._lrm_kw(lr=self.lr_dev, wd=self._wd_scalar(e.seg) if self.seg_wd is not None else 0.0)
            (be.dense_dw_adam_fin_lrmul if fin else be.dense_dw_adam_lrmul)(*args, self._lrm_scalar(e.seg), **kw,
                                                                            guard=self._guard_word())
        elif self._gclip() is not None:
            kw = self._gclip_kw(lr=self.lr_dev, wd=self._wd_scalar(e.seg) if self.seg_wd is not None else 0.0)
            (be.dense_dw_adam_fin_gclip if fin else be.dense_dw_adam_gclip)(*args, **kw, guard=self._guard_word())
        elif self.seg_wd is None:
            (be.dense_dw_adam_fin if fin else be.dense_dw_adam)(*args, guard=self._guard_word())
        else:
            (be.dense_dw_adamw_fin if fin else be.dense_dw_adamw)(*args, self.lr_dev, self._wd_scalar(e.seg),
                                                                  guard=self._guard_word())

    def _sgd_update(self, spans):
        """clip + SGD over ``spans``: tnt_sgd_f32 / tnt_sgdw_f32 (its learning rate comes from the device only)"""
        be, a, opt = self.be, self.arena, self.optimizer
        seg, off, length, nspan = spans
        args = (a.theta, self.opt_m, a.grad, seg, off, length, a.seg_l2, a.sq, a.sq_override, nspan)
        if self.seg_lrm is not None:
            be.sgd_lrmul(*args, 0.0, self.lr_dev, opt.momentum, self._clip(), self.seg_lrm, **self._lrm_kw(seg_wd=self.seg_wd),
                         guard=self._guard_word())
        elif self._gclip() is not None:
            be.sgd_gclip(*args, 0.0, self.lr_dev, opt.momentum, self._clip(), **self._gclip_kw(seg_wd=self.seg_wd),
                         guard=self._guard_word())
        elif self.seg_wd is None:
            be.sgd(*args, 0.0, self.lr_dev, opt.momentum, self._clip(), guard=self._guard_word())
        else:
            be.sgdw(*args, self.lr_dev, opt.momentum, self._clip(), self.seg_wd, guard=self._guard_word())

    def _average_update(self):
        """The averaging launch of a step (tnt_weight_average_f32 over the whole arena): the step's last launch, behind its
        last update launch and inside the same recorded plan / graph.  Copy, skip or blend is decided on the device from
        adam_t, which must equal the number of applied updates by then, and from the guard word.  Nothing without an
        averaging optimizer."""
        av = self.average
        if av is None:
            return
        a = self.arena
        self.be.weight_average(a.theta, self.opt_avg, a.total, self.adam_t, av.kind_id, av.momentum, av.dynamic, av.start_step,
                               av.every, guard=self._guard_word())

    def _update_fused(self, l2_out, skip_first=False):
        """single-process update: [AGC] -> span norms -> ONE finalize launch (per-variable norms, L2 metric, the step's
        loss / accuracy totals if the model deferred them, step tick) -> clip + Adam / SGD.  Replaces the five dependent
        launches seg_finalize, l2_total, sum2, step_tick of the unfused sequence (each ~4.6 us inside the graph).
        ``skip_first`` (dp.PipelinedDenseSync with a row-sharded encoder kernel): variable 0 is updated by the caller, its
        (sum g^2, sum theta^2) pair sits in partial[0:2] with the variable's other slots zero -- the finalize work files it
        like any other, the norm / update launches here start behind it.
        Three phases: the norm launch(es) (_fused_norms), the finalize arguments (_finalize_args), the update launches
        (_fused_updates).  The step's tail (StepTail) is taken here and left empty."""
        sp, adam = self.arena.spans, self.optimizer.kind == "adam"
        self._apply_agc()
        tail, self._tail = self._tail, StepTail()
        enc = tail.enc
        # lr_dev is first read by the norm launch that carries the lr job, else by the finalize launch: the schedule goes here
        self._lr_schedule_launch()
        s1 = 0          # the first span the norm / update launches here walk
        if skip_first:
            if enc is not None or not adam:
                raise RuntimeError("skip_first needs Adam and an encoder gradient that the caller handles")
            s1 = sp.first_host[1]
        if enc is not None:
            s1 = sp.first_host[self.arena.entries[enc.name].seg + 1]
        # no finalize launch (tnt_adam_fin_f32): the norm launch leaves lr_t, the update launches sum the clip norms they need
        # from the span partials themselves, one extra workgroup of the Adam launch files the scalars, the counters tick at its end
        fin = adam and hasattr(self.be, "adam_fin") and self.fused_finalize
        fin = self._fused_norms(enc, s1, fin)
        self._fused_updates(l2_out, enc, s1, fin, self._finalize_args(tail))

    def _fused_norms(self, enc, s1, fin):
        """_update_fused, phase 1: the norm partials of every variable's spans from span ``s1`` on, and of the encoder
        kernel handed over in ``enc``.  ``fin``: the launch also carries Adam's lr job (lr_t from the step counter) for an
        update without a finalize launch.  Returns whether it did: False where a plain span_sqnorm ran."""
        be, a, opt = self.be, self.arena, self.optimizer
        seg, off, length, nspan = self._spans(s1)
        lr_job = (self.adam_t, self.lr_dev, self.lr_t_dev, opt.beta_1, opt.beta_2) if fin else None
        # the norm launch reads only what the update will consume (tnt_span_norm, csrc/tnt_fin.h): no gradient pass for a
        # variable whose clip norm is supplied through sq_override, no theta pass where there is no regulariser
        skip = a.sq_override if (fin and not self.agc) else None
        if enc is not None:
            # The dense encoder kernel (segment 0, 59 % of config 2's parameters) never has its gradient written: one
            # pass of the skinny product leaves its norm partials in the variable's span slots, a second one applies
            # clip + Adam to the strips as they leave the MFMAs (24 bytes per parameter instead of 40).
            e, g = a.entries[enc.name], enc.gram
            if g is not None and 4 * enc.rows + g.nw2 <= s1 and self.seg_lrm is not None:
                # with a multiplier table the Gram-norm launch runs alone: the span norms that ride in it would read a frozen
                # variable's gradient, so they run in the table form of the norm launch below
                be.dense_gram_norm(enc.dpre, g.pre, g.bias, g.gx, g.nsplit, g.w2, g.nw2, e.l2, a.partial, s1, enc.rows, enc.E)
            elif g is not None and 4 * enc.rows + g.nw2 <= s1:
                # norm from the forward's by-products: ||X^T D||^2 = sum (X X^T) o (D D^T), no pass over the gradient
                # ... with the span norms of every other variable riding in the same launch
                be.dense_gram_norm(enc.dpre, g.pre, g.bias, g.gx, g.nsplit, g.w2, g.nw2, e.l2, a.partial, s1, enc.rows, enc.E,
                                   spans=(a.theta, a.grad, seg, off, length, a.seg_l2, a.partial[2 * s1:], nspan),
                                   lr_job=lr_job, skip=skip)
                return fin
            else:
                be.dense_dw_sqnorm(enc.x, enc.dpre, a.p(enc.name), e.l2, a.partial, s1, enc.N, enc.E, enc.rows, enc.ldx)
        if self.seg_lrm is not None:
            # the forms that do not read a frozen variable's gradient, with or without the lr job
            fin = bool(fin and nspan > 0)
            be.span_sqnorm_lrmul(a.theta, a.grad, seg, off, length, a.seg_l2, a.partial[2 * s1:], nspan, self.seg_lrm,
                                 lr_job=lr_job if fin else None, skip=skip if fin else None)
            return fin
        if fin and nspan > 0:
            be.span_sqnorm_lr(a.theta, a.grad, seg, off, length, a.seg_l2, a.partial[2 * s1:], nspan, *lr_job, skip=skip)
            return True
        be.span_sqnorm(a.theta, a.grad, seg, off, length, a.seg_l2, a.partial[2 * s1:], nspan)
        return False

    def _finalize_args(self, tail):
        """_update_fused, phase 2: the keywords of the step's finalize work -- what the step handed over in ``tail`` and the
        step state that ticks -- for whichever launch carries it (finalize_desc of the Adam launch, or step_finalize)"""
        opt, adam = self.optimizer, self.optimizer.kind == "adam"
        return dict(tail.finalize_kw(), adam_t=self.adam_t, drop_step=self.drop_step, lr=self.lr_dev,
                    lr_t=self.lr_t_dev if adam else None, beta1=opt.beta_1 if adam else 0.0,
                    beta2=opt.beta_2 if adam else 0.0, guard=self._guard_word())

    def _fused_updates(self, l2_out, enc, s1, fin, kw):
        """_update_fused, phase 3: the finalize work ``kw`` (_finalize_args) and clip + Adam / SGD from span ``s1`` on, the
        encoder kernel's fused update (``enc``) included.  ``fin``: inside the Adam launch (its descriptor), else as the
        step_finalize launch in front of the update launches."""
        be, a, sp = self.be, self.arena, self.arena.spans
        spans = self._spans(s1)
        if fin:
            if "extra_part" in kw:
                kw["extra_seg"] = self.emb_seg
            self._global_sqnorm(kw)    # global_clipnorm: the one word both update launches clip by, from the span partials
            if enc is not None:        # the encoder kernel first: it reads the step counter's lr_t like the Adam launch, which ticks
                self._enc_adam_update(enc, fin=True)
            if self._fin_arrive is None:
                self._fin_arrive = torch.zeros(16, dtype=torch.int32, device=self.device)
            # one descriptor per distinct argument set, alive as long as the model (recorded launch plans re-issue the call)
            ck = tuple((k, v.data_ptr() if torch.is_tensor(v) else v) for k, v in sorted(kw.items())) + (l2_out.data_ptr(),)
            if ck not in self._fin_descs:
                self._fin_descs[ck] = be.finalize_desc(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, l2_out, a.nseg,
                                                       self._fin_arrive, **kw)
            self._adam_fin_update(spans, self._fin_descs[ck], self._ring_args())
            # the counters tick when the last workgroup of the Adam launch arrives, behind the encoder's update: adam_t is
            # the number of applied updates when the averaging launch starts
            self._average_update()
            return
        be.step_finalize(a.partial, sp.seg_first, a.seg_l2, a.sq, a.wsq, l2_out, a.nseg, **kw)
        self._global_sqnorm()
        if self.optimizer.kind == "adam":
            self._adam_update(spans, self._ring_args() if spans[3] > 0 else None)
            if enc is not None:
                self._enc_adam_update(enc, fin=False)
        else:
            self._sgd_update(spans)
        # the finalize launch ticked in front of the update launches: adam_t is the number of applied updates here too
        self._average_update()

    # ------------------------------------------------------------------ BatchNorm, optionally synchronised across replicas
    def _sync_bn_on(self):
        """Synchronised BatchNorm (``sync_bn = True`` on a data-parallel model): batch statistics over the GLOBAL batch, so
        G replicas x local batch train exactly like one process on the concatenated batch.  The reference has no
        counterpart (it trains on one device); per-replica statistics remain the default.  The collectives sit inside
        the forward / backward pass, so dp.attach puts such a model on the generic (non-pipelined, eager) schedule."""
        return bool(self.sync_bn and self.dp_world > 1)

    def _bn_fwd(self, x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, C, ldy, training, work, drop=None):
        """drop = (rate, seed, site, step_dev), training only: the Dropout over y that follows the normalisation, fused into
        the apply pass where the backend offers it (returns True when it was applied)"""
        be = self.be
        if not (training and self._sync_bn_on()):
            if drop is not None and drop[0] > 0 and self.fused_bn_drop:
                be.batchnorm_fwd(x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, C, ldy, training, BN_EPS,
                                 BN_MOMENTUM, work, drop=drop)
                return True
            be.batchnorm_fwd(x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, C, ldy, training, BN_EPS, BN_MOMENTUM,
                             work)
            return False
        import torch.distributed as dist
        n = be.bn_nchunk(rows) * 2 * C
        part, allp = work[C:C + n], self._bn_scratch(self.dp_world * n)
        be.batchnorm_stats(x, rows, C, part)
        dist.all_gather(list(allp.view(self.dp_world, n).unbind(0)), part.contiguous())
        be.batchnorm_apply_stats(allp, self.dp_world, x, gamma, beta, mov_mean, mov_var, y, xhat, inv_std, rows, C, ldy, BN_EPS,
                                 BN_MOMENTUM, work)

    def _bn_bwd(self, dy, xhat, gamma, inv_std, dx, dgamma, dbeta, rows, C, lddy, work, act_pre=None, slope=0.2):
        """act_pre: LeakyReLU' of the activation in front of the normalisation folded into the dx pass (returns True when
        it was applied)"""
        be = self.be
        if not self._sync_bn_on():
            if act_pre is not None and self.fused_bn_drop:
                be.batchnorm_bwd(dy, xhat, gamma, inv_std, dx, dgamma, dbeta, rows, C, lddy, True, work, act_pre=act_pre,
                                 slope=slope)
                return True
            be.batchnorm_bwd(dy, xhat, gamma, inv_std, dx, dgamma, dbeta, rows, C, lddy, True, work)
            return False
        import torch.distributed as dist
        # local sums stay in the gradient buffers (the replicas' gradients are averaged as usual); dx needs the global sums
        be.batchnorm_bwd(dy, xhat, gamma, inv_std, None, dgamma, dbeta, rows, C, lddy, True, work)
        sums = self._bn_scratch(2 * C)
        sums[:C].copy_(dgamma.reshape(-1)[:C]); sums[C:2 * C].copy_(dbeta.reshape(-1)[:C])
        dist.all_reduce(sums[:2 * C], op=dist.ReduceOp.SUM)
        be.batchnorm_dx(dy, lddy, xhat, gamma, inv_std, sums[:C], sums[C:2 * C], dx, rows, C, rows * self.dp_world)

    def _bn_scratch(self, n):
        buf = self._bn_buf
        if buf is None or buf.numel() < n:
            buf = self._bn_buf = self._f(n)
        return buf[:n]

    def _emb_sparse_ok(self, E, ldd):
        """the sparse Embedding backward runs (single-process fused step)"""
        return bool(self._tail.deferring and self.dp_world == 1 and self.sparse_emb_bwd and E % 4 == 0 and ldd % 4 == 0)

    def _embedding_bwd(self, drows, ids, name, B, T, E, ldd, V, zero_id=-1):
        """Embedding scatter + IndexedSlices norm.  Inside the fused single-process step (_deferring) the sparse
        form runs: no table-wide zero fill (rows touched by the previous step only are cleaned through ``prev_ids``),
        the norm as per-block partials that the step-finalize launch sums.  Anywhere else (data parallel: the all-reduce
        writes rows of other ranks' tokens; SAM; eager paths) the dense form runs and hands its ids on as prev_ids, so
        the invariant "dtable is zero outside the rows of prev_ids" holds whichever form runs next."""
        be, a = self.be, self.arena
        if self._skip_grad(name):       # a frozen Embedding: neither the scatter nor its un-deduplicated norm
            return
        seg = a.entries[name].seg
        sqo = a.sq_override[seg:seg + 1]
        st = self._emb_state
        if st is None or st[0] != (B, T, name):
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("embedding backward state must be built outside a graph capture (run one eager step)")
            nparts = be.embedding_bwd_parts(B, T, E)
            st = self._emb_state = ((B, T, name), torch.full((B * T,), -1, dtype=torch.int32, device=self.device),
                                    self._f(nparts), nparts)
            a.g(name).zero_()
        _, prev, parts, nparts = st
        sparse = self._emb_sparse_ok(E, ldd)
        if sparse:
            # rows of the mask id carry no gradient (the caller's guarantee): not read
            kw = dict(zero_id=zero_id) if zero_id >= 0 else {}
            be.embedding_bwd_sparse(drows, ids, prev, a.g(name), parts, B, T, E, ldd, V, **kw)
            # the finalize work hands this step's ids on as prev_ids and sums the norm partials (not under AGC: its launch
            # writes the clipped rows' norm into the variable's sq_override slot itself)
            t = self._tail
            t.ids_src, t.ids_dst, t.n_ids = ids, prev, B * T
            if not self.agc:
                t.extra_part, t.extra, t.n_extra = parts, sqo, nparts
        else:
            be.embedding_bwd(drows, ids, a.g(name), sqo, self.rowsq, B, T, E, ldd, V)
            prev.copy_(ids.reshape(-1))

    def _sum2(self, x0, out0, x1, out1, n, scale):
        """loss / accuracy totals: deferred into the step-finalize launch when a fused update follows in the same
        launch sequence (inside _deferring), else their own launch"""
        if self._tail.deferring:
            t = self._tail
            t.x0, t.out0, t.x1, t.out1, t.n, t.scale = x0, out0, x1, out1, n, scale
        else:
            self.be.sum2(x0, out0, x1, out1, n, scale)

    def _tick(self):
        """the schedule's launch and the step tick of an update without a finalize launch (_apply_optimizer, and once per
        step in front of the first _update_slice)"""
        opt, gd = self.optimizer, self._guard_word()
        self._lr_schedule_launch()
        if opt.kind == "adam":
            self.be.step_tick(self.adam_t, self.drop_step, self.lr_dev, self.lr_t_dev, opt.beta_1, opt.beta_2, guard=gd)
        else:
            self.be.step_tick(self.adam_t, self.drop_step, self.lr_dev, None, 0.0, 0.0, guard=gd)

    def _update_slice(self, sl):
        """norms + clip + optimizer on one contiguous range of variables (arena.seg_slice); the caller
        runs _tick() once before the first slice and l2_total after the last."""
        a, spans = self.arena, (sl.span_seg, sl.span_off, sl.span_len, sl.nspan)
        self.be.seg_sqnorm(a.theta, a.grad, *spans[:3], sl.seg_first, a.seg_l2, sl.partial, sl.sq, sl.wsq, None, sl.nspan, sl.nseg)
        if self.optimizer.kind == "adam":
            self._adam_update(spans)
        else:
            self._sgd_update(spans)

    @staticmethod
    def pick_splitk(M, N, K):
        """Split-K factor (power of two) so that a GEMM launches ~1024 workgroups of 64x64 tiles
        (4 per CU), calibrated with tools/gemm_bench.py: head dX (120 tiles) -> 8, dXin (128) -> 8,
        dU (256) -> 4, head dW (632) -> 2, encoder forward (8 tiles, K = 20000) -> 64."""
        tiles = ((M + 63) // 64) * ((N + 63) // 64)
        if K < 256:
            return 1
        sk = 1
        while sk * 2 * tiles <= 1280 and K // (sk * 2) >= 128 and sk < 64:
            sk *= 2
        return sk

    def _alloc_splitk(self, shapes):
        """Workspace for the split-K GEMMs of this model: shapes = [(M, N, K), ...]."""
        need = max([self.pick_splitk(*s) * s[0] * s[1] for s in shapes] + [1])
        self.skwork = self._f(need)

    def _g3_space(self, floats):
        """Split-K exchange space of tnt_gemm3_f32: ONE armed work buffer and ONE error word per model, shared by every
        launch (launches of a model run one after the other on its stream, and every launch leaves the buffer armed).
        Grown during eager passes only; growing invalidates captured graphs."""
        w, sy = self._g3_work, self._g3_sync
        if w is None or w.numel() < floats or sy is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("gemm3 split-K workspace too small inside a graph capture (run one eager step first)")
            if w is None or w.numel() < floats:
                w = self._g3_work = self._f((max(floats, 4) + 3) // 4 * 4)
                self.be.gemm3_work_arm(w)
            if sy is None:
                sy = self._g3_sync = torch.zeros(64, dtype=torch.int32, device=self.device)
            self._graphs = {}
        return w, sy

    def _g3_plan(self, M, N, K, transA, transB, batch, colsum):
        key = (M, N, K, bool(transA), bool(transB), batch, bool(colsum))
        plans = self._g3_plans
        if key not in plans:
            force = (self.g3_force or {}).get(key[:6])          # tools / tests: {(M, N, K, tA, tB, batch): (tile, splitk)}
            plans[key] = force or self.be.gemm3_plan(M, N, K, transA, transB, batch, allow_split=not colsum)
        return plans[key]

    def gemm3(self, A, B, C, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, colsum=None, A2=None, C2=None,
              live=None, live_mode=0, plan_M=None):
        """One product (or two sharing B) on the hand-written FP32-MFMA family of csrc/gemm3.hip, tile and K split from the
        library's cost model (tnt_gemm3_plan; cached per shape).  True = call issued.
        ``live`` / ``live_mode`` (ops.LIVE_ROWS_M / LIVE_ROWS_K): a device word that bounds the rows (tnt_gemm3_f32);
        ``plan_M``: the extent to EXPECT in that word -- the tile is planned for it (unsplit: the grid still covers M, and
        the splits of a tile would have to be resident together), the result never depends on it."""
        be = self.be
        if not self.use_gemm3 or not hasattr(be, "gemm3") or (transA and transB):
            return False
        if lda % 4 or ldb % 4 or ldc % 4:
            return False
        batch = 2 if A2 is not None else 1
        if plan_M is not None and live is not None and plan_M < M:
            tile, sk = self._g3_plan(plan_M, N, K, transA, transB, batch, True)
        else:
            tile, sk = self._g3_plan(M, N, K, transA, transB, batch, colsum is not None)
        work, sync = self._g3_space(be.gemm3_work_floats(M, N, tile, sk, batch)) if sk > 1 else (None, None)
        kw = dict(live=live, live_mode=live_mode) if live is not None else {}
        be.gemm3(A, B, C, M, N, K, lda, ldb, ldc, transA=transA, transB=transB, bias=bias, colsum=colsum, A2=A2, C2=C2,
                 tile=tile, splitk=sk, work=work, sync=sync, **kw)
        return True

    def _g3_pair_live(self, p, q):
        """a pair launch planned for the rows expected to exist: the switch is on, the backend has the joint plan and a
        product carries a live word with its expected extent (``plan_M``)"""
        return (self.g3_live_map and hasattr(self.be, "gemm3_plan_pair")
                and any(d.get("plan_M") is not None and d.get("live") is not None for d in (p, q)))

    def _g3_plan_pair(self, p, q):
        """the joint plan of a pair launch whose products carry ``plan_M`` (tnt_gemm3_plan_pair; cached per argument set):
        ((tile, splitk), (tile, splitk)), or None -- not such a launch (_g3_pair_live), a forced plan, or independent picks
        without a pair form -- for the two independent plans"""
        from .ops import G3_PLAN_MAP, G3_PLAN_NOSPLIT, G3_PLAN_SMALL, LIVE_ROWS_M
        be = self.be
        if not self._g3_pair_live(p, q):
            return None
        args = []
        for d in (p, q):
            live = d.get("plan_M") if d.get("live") is not None else None
            flags = (G3_PLAN_NOSPLIT if d.get("colsum") is not None else 0) | (G3_PLAN_SMALL if d.get("small") else 0) \
                | (G3_PLAN_MAP if d.get("live_mode") == LIVE_ROWS_M else 0)
            args.append((d["M"], d["N"], d["K"], int(d.get("transA", False)), int(d.get("transB", False)),
                         2 if d.get("A2") is not None else 1, int(live or 0), flags))
        forced = self.g3_force or {}
        if any((a[0], a[1], a[2], bool(a[3]), bool(a[4]), a[5]) in forced for a in args):
            return None                 # a forced plan (tools, tests) stands
        key = ("pair",) + tuple(args)
        plans = self._g3_plans
        if key not in plans:
            r = be.gemm3_plan_pair(*args)
            plans[key] = None if r is None else (r[0][:2], r[1][:2])
        return plans[key]

    def gemm3_pair(self, p, q):
        """Two INDEPENDENT products in one launch (tnt_gemm3_pair_f32): p, q = dicts of gemm3's arguments.  True = issued;
        False = this pair has no co-launch form (the caller issues the two products itself).
        ``plan_M`` in a dict: the extent to EXPECT in that product's live word (rows for LIVE_ROWS_M, the contraction for
        LIVE_ROWS_K).  With it (``g3_live_map``) the two products are planned together for the work they will really do
        (_g3_plan_pair) and a split LIVE_ROWS_M product deals its grid over the live rows only (LIVE_ROWS_M_MAP); the
        result never depends on the value."""
        from .ops import LIVE_ROWS_M, LIVE_ROWS_M_MAP
        be = self.be
        if not self.use_gemm3 or not hasattr(be, "gemm3_pair"):
            return False
        live_map = self._g3_pair_live(p, q)
        joint = self._g3_plan_pair(p, q)
        descs, need = [], 0
        for i, d in enumerate((p, q)):
            if d["lda"] % 4 or d["ldb"] % 4 or d["ldc"] % 4:
                return False
            batch = 2 if d.get("A2") is not None else 1
            if joint is not None:
                tile, sk = joint[i]
            else:
                tile, sk = self._g3_plan(d["M"], d["N"], d["K"], d.get("transA", False), d.get("transB", False), batch,
                                         d.get("colsum") is not None)
                if d.get("small"):            # a small product rides along: the 32-deep tile of the SAME shape has a pair form
                    tile = {9: 7, 10: 5}.get(tile, tile)      # (same tile count, so the planned split stays valid)
            wf = (be.gemm3_work_floats(d["M"], d["N"], tile, sk, batch) + 3) // 4 * 4 if sk > 1 else 0
            descs.append((d, tile, sk, need, wf))
            need += wf
        (d1, t1, _, _, _), (d2, t2, _, _, _) = descs
        if not be.gemm3_pair_supported(t1, d1.get("transA", False), d1.get("transB", False), t2, d2.get("transA", False),
                                       d2.get("transB", False)):
            return False
        work, sync = self._g3_space(need) if need else (None, None)
        # the descriptors are passed by address and recorded launch plans re-issue the call later: one descriptor pair per
        # distinct argument set, kept for the life of the model (same operands -> same objects)
        ck = tuple((tuple((k, v.data_ptr() if torch.is_tensor(v) else v) for k, v in sorted(d.items()) if k not in ("small", "plan_M")), tile, sk, off,
                    live_map)
                   for d, tile, sk, off, _ in descs) + (work.data_ptr() if need else 0,)
        keep = self._g3_descs
        if ck in keep:
            be.gemm3_pair(*keep[ck])
            return True
        out = []
        for d, tile, sk, off, wf in descs:
            lv = dict(live=d["live"], live_mode=d["live_mode"]) if d.get("live") is not None else {}
            if live_map and sk > 1 and lv.get("live_mode") == LIVE_ROWS_M:
                lv["live_mode"] = LIVE_ROWS_M_MAP
            out.append(be.gemm3_desc(d["A"], d["B"], d["C"], d["M"], d["N"], d["K"], d["lda"], d["ldb"], d["ldc"],
                                     transA=d.get("transA", False), transB=d.get("transB", False), bias=d.get("bias"),
                                     colsum=d.get("colsum"), A2=d.get("A2"), C2=d.get("C2"), tile=tile, splitk=sk,
                                     work=work[off:off + wf] if wf else None, sync=sync if wf else None, **lv))
        keep[ck] = (out[0], out[1])
        be.gemm3_pair(out[0], out[1])
        return True

    def _route_lt(self, A, B, C, M, N, K, lda, ldb, ldc, ws, kw):
        """A/B tool since round 3 (``use_gemm3 = False``): hipBLASLt (tnt_gemm_lt_f32) for the vocabulary-sized GEMMs, i.e. the
        head forward and its two gradients; rocBLAS for the LSTM-sized ones (gemm_sk below).  True = call issued."""
        be = self.be
        if (not hasattr(be, "gemm_lt") or kw.get("pre") is not None or kw.get("act", 0)
                or kw.get("accumulate") or max(N, K) < 4096 or 2.0 * M * N * K < self.lt_min_flops):
            return False
        tA, tB = bool(kw.get("transA", False)), bool(kw.get("transB", False))
        if tA and tB:
            return False
        be.gemm_lt(A, B, C, M, N, K, lda, ldb, ldc, transA=tA, transB=tB, bias=kw.get("bias"))
        return True

    def gemm_sk(self, A, B, C, M, N, K, lda, ldb, ldc, ws=0, **kw):
        """GEMM with the calibrated split-K choice.  ``ws`` selects the split-K workspace (one per
        concurrent branch, see ``side``).  Workspaces grow on demand during eager (warm-up) passes;
        growing one invalidates captured graphs, which are then re-captured."""
        # default since round 3: every product without an activation epilogue that is large enough to fill the chip runs on
        # the hand-written family (csrc/gemm3.hip); the vendor libraries remain as A/B tools (use_gemm3 = False)
        if (kw.get("pre") is None and kw.get("act", 0) == 0 and not kw.get("accumulate") and 2.0 * M * N * K >= self.g3_min_flops
                and self.gemm3(A, B, C, M, N, K, lda, ldb, ldc, transA=kw.get("transA", False), transB=kw.get("transB", False),
                               bias=kw.get("bias"))):
            return
        if not self.use_gemm3 and self._route_lt(A, B, C, M, N, K, lda, ldb, ldc, ws, kw):
            return
        plain = kw.get("bias") is None and kw.get("pre") is None and kw.get("act", 0) == 0
        # One shape family where the vendor's pick is poor: NT with a narrow output and a very long K (config 3's
        # head dX = dlogits[960x5001] @ Wo^T[5001x256]: 59 us = 42 TF, against 38 us for the tiled kernel with
        # split-K 16; tools/c3_head_grad_probe.py).  At N = 512 the two are level and the library stays.
        blas_poor = kw.get("transB", False) and not kw.get("transA", False) and N <= 256 and K >= 16 * N
        if (plain and not blas_poor and self.use_blas and not self.use_gemm3
                and hasattr(self.be, "gemm_blas")):
            # no fused epilogue (weight / input gradients): the vendor's stream-K sgemm (tnt_gemm_blas_f32) needs no
            # split-K pass + reduce launch on these skinny-output / long-K shapes
            self.be.gemm_blas(A, B, C, M, N, K, lda, ldb, ldc, transA=kw.get("transA", False),
                              transB=kw.get("transB", False), accumulate=kw.get("accumulate", False))
            return
        sk = self.pick_splitk(M, N, K)
        if sk > 1:
            pool = self._skw
            buf = self.skwork if ws == 0 else pool.get(ws)
            if buf is None or sk * M * N > buf.numel():
                if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("split-K workspace too small inside a graph capture")
                buf = self._f(sk * M * N)
                if ws == 0:
                    self.skwork = buf
                else:
                    pool[ws] = buf
                self._graphs = {}
            self.be.gemm(A, B, C, M, N, K, lda, ldb, ldc, splitk=sk, work=buf, **kw)
        else:
            self.be.gemm(A, B, C, M, N, K, lda, ldb, ldc, **kw)

    # ---- intra-step concurrency: independent gradient GEMMs run on side streams (captured as parallel
    # graph branches) next to the latency-bound BPTT chain, which leaves most CUs idle.
    @contextmanager
    def side(self, i):
        # Measured on MI355X (tools/side_bench.py): 0.868 ms/step without, 0.94-1.07 ms with side branches --
        # the concurrent GEMM workgroups crowd out the LDS-heavy BPTT step kernels.  Off by default.
        if i < 0 or self.device.type != "cuda" or not self.use_side_streams:
            yield
            return
        streams = self._side_streams
        if i not in streams:
            streams[i] = torch.cuda.Stream(device=self.device)
        s = streams[i]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            yield
        self._side_used.add(i)

    def join(self):
        used = self._side_used
        if not used:
            return
        main = torch.cuda.current_stream()
        for i in sorted(used):
            main.wait_stream(self._side_streams[i])
        used.clear()

    # ------------------------------------------------------------------ adaptive gradient clipping (agc.py)
    def enable_agc(self, clip_factor=0.01, eps=1e-3):
        """gradients = agc.adaptive_clip_grad(trainable_variables, gradients, clip_factor, eps) before
        optimizer.apply_gradients -- the (commented-out) call of lc_NIC.py:388.  clip_factor=None switches it off."""
        compat.check(self, ("agc",), agc=clip_factor is not None)
        self.agc = None if clip_factor is None else (float(clip_factor), float(eps))
        self._graphs = {}

    def _emb_row_grads(self):
        """(row-gradient matrix of the Embedding [n][E], n, E, ld, arena name) or None: the IndexedSlices values whose
        un-deduplicated column norms agc.py:25-30 uses.  Set by the models that have an Embedding."""
        return self._route.emb_rows

    def _apply_agc(self):
        if not self.agc:
            return
        from .arena import AgcTable
        a, er = self.arena, self._emb_row_grads()
        tab = self._agc_tab
        if tab is None:
            shapes = {n: self.keras_shapes[n] for n in a.entries}
            tab = self._agc_tab = AgcTable(a, shapes, er[4] if er else None)
            self._agc_colsq = self._f(er[2]) if er else None
        if er is not None:
            x, n, E, ld, name = er
            self.be.colsq(x, self._agc_colsq, n, E, ld)
            seg = a.entries[name].seg
            self.be.agc(a.theta, a.grad, tab, self._agc_colsq, a.sq_override[seg:seg + 1], *self.agc)
        else:
            self.be.agc(a.theta, a.grad, tab, None, None, *self.agc)

    def _norms_and_l2(self, l2_out):
        a, sp = self.arena, self.arena.spans
        args = (a.theta, a.grad, sp.span_seg, sp.span_off, sp.span_len, sp.seg_first, a.seg_l2, a.partial, a.sq, a.wsq, l2_out,
                sp.nspan, a.nseg)
        if self.seg_lrm is not None:       # a frozen variable's gradient is not read
            self.be.seg_sqnorm_lrmul(*args, self.seg_lrm)
        else:
            self.be.seg_sqnorm(*args)

    # ------------------------------------------------------------------ weights
    def _state_map(self):
        """keras name -> device tensor of the variables kept outside the arena (BatchNorm moving statistics), in the order
        dp.py broadcasts them"""
        return {}

    def state_tensors(self):
        """Non-trainable device state (BatchNorm moving statistics)."""
        return list(self._state_map().values())

    def set_weight(self, name, arr):
        arr = np.asarray(arr, dtype=np.float32)
        assert tuple(arr.shape) == tuple(self.keras_shapes[name]), (name, arr.shape, self.keras_shapes[name])
        dst = self._state_map().get(name)
        if dst is None:
            dst = self.arena.p(name)
        dst.copy_(torch.from_numpy(pack(arr, dst.shape, name)))

    def _unpack(self, name, t):
        return unpack(t.detach().cpu().numpy(), self.keras_shapes[name], name)

    def get_weight(self, name):
        t = self._state_map().get(name)
        return self._unpack(name, self.arena.p(name) if t is None else t)

    def get_gradient(self, name):
        """Last computed gradient of a trainable (keras layout, *without* the L2 term, which the
        optimizer kernels add on the fly).  Under gradient accumulation: behind a closing micro-step what the update
        consumed, the window's mean gradient; behind any other that micro-batch's share of it (its gradient / k).
        A frozen variable has no gradient: ValueError."""
        self._frozen_gradient_refuse(name)
        return self._unpack(name, self.arena.g(name))

    def _frozen_gradient_refuse(self, name):
        if self._frozen(name):
            raise ValueError(f"{name} is frozen: a frozen variable's gradient is undefined (its buffer holds whatever an "
                             "earlier step left)")

    @property
    def losses(self):
        """[lambda*||W||^2 ...] as self.losses (NIC.py:242-243)."""
        a = self.arena
        self._norms_and_l2(self.met[2:3])
        return [a.seg_l2[e.seg] * a.wsq[e.seg] for e in a.entries.values() if e.l2 > 0]

    @property
    def trainable_variables(self):
        return [(n, self.get_weight(n)) for n in self.trainable_names()]

    def trainable_names(self):
        """the variables a training step updates: not the BatchNorm moving statistics, not the frozen ones"""
        return [n for n in self.keras_shapes if "moving_" not in n and not self._frozen(n)]

    def non_trainable_names(self):
        """the rest: the frozen variables and the BatchNorm moving statistics"""
        return [n for n in self.keras_shapes if "moving_" in n or self._frozen(n)]

    def get_weights_dict(self):
        return OrderedDict((n, self.get_weight(n)) for n in self.keras_shapes)

    def set_weights_dict(self, d, strict=True):
        for n, v in d.items():
            if n in self.keras_shapes:
                self.set_weight(n, v)
            elif strict:
                raise KeyError(n)

    def get_optimizer_slot(self, name, slot):
        """Adam first ('m') / second ('v') moment (SGD: 'm' = momentum) of one trainable, or its weight average
        ('average', with optimizers.MovingAverage / SWA; the same values while it is swapped in), in the keras layout."""
        if slot == "average":
            buf = self._average_buf("get_optimizer_slot(..., 'average')")
            buf = self.arena.theta if self._swapped else buf
        else:
            buf = self.opt_m if slot == "m" else self.opt_v
        return self._unpack(name, self.arena.slot(buf, name))

    # ------------------------------------------------------------------ weight average (optimizers.MovingAverage / SWA)
    def _average_buf(self, what):
        """opt_avg; ValueError on a model compiled without averaging"""
        if self.average is None:
            raise ValueError(f"{what} needs a model compiled with an averaging optimizer (optimizers.MovingAverage / SWA)")
        if self.opt_avg is None:
            raise RuntimeError(f"{what}: the average exists once the optimizer state does, from the first training step on")
        return self.opt_avg

    def swap_weights(self):
        """Exchanges the weights and their average in place (tnt_swap_f32): what every launch reads as the weights is the
        average until the next call.  Captured graphs and launch plans hold the buffers' addresses, so the contents move,
        not the tensors, and nothing is re-captured; no decode or evaluation path keeps a buffer derived from the weights
        across calls.  BatchNorm moving statistics are not averaged and stay.  While swapped a training step is refused."""
        avg = self._average_buf("swap_weights")
        self.be.swap(self.arena.theta, avg, self.arena.total)
        self._swapped = not self._swapped

    @contextmanager
    def averaged_weights(self):
        """``with model.averaged_weights():`` predict / evaluate with the averaged weights: swaps in, and swaps back on the
        way out, also on an exception."""
        self._average_buf("averaged_weights")
        if self._swapped:
            raise RuntimeError("the averaged weights are already swapped in")
        self.swap_weights()
        try:
            yield self
        finally:
            self.swap_weights()

    def assign_average_vars(self):
        """tfa's name: the average becomes the weights (a copy; the average stays), for the end of training."""
        avg = self._average_buf("assign_average_vars")
        if self._swapped:
            raise RuntimeError("the averaged weights are swapped in: swap back before assign_average_vars")
        self.arena.theta.copy_(avg)

    def get_layer(self, name):
        if name not in self.layers_spec:
            raise ValueError(f"No such layer: {name}")
        return _LayerView(self, name, self.layers_spec[name])

    def save_weights(self, path, averaged=False):
        """ModelCheckpoint(save_weights_only=True) target (main.py:168-190).  ``averaged=True`` (optimizers.MovingAverage /
        SWA): the trainables are written from their weight average, BatchNorm moving statistics as they are.  ``*.h5`` / ``*.hdf5``: a Keras weight file
        (layer_names / weight_names attributes, one float32 dataset per weight, keras layouts), written by the
        pure-Python h5lite module -- readable by h5py / Keras ``load_weights(by_name=True)`` wherever the layer names
        agree.  Anything else: ``.npz`` with the same names and layouts."""
        path = str(path)
        get = self.get_weight
        if averaged:
            self._average_buf("save_weights(averaged=True)")
            get = lambda n: self.get_optimizer_slot(n, "average") if n in self.arena.entries else self.get_weight(n)
        if path.endswith((".h5", ".hdf5")):
            from . import h5lite
            layers = OrderedDict((layer, [(f"{layer}/{w}:0", get(f"{layer}/{w}")) for w in ws])
                                 for layer, ws in self.layers_spec.items())
            h5lite.write_keras_weights(path, layers)
            return
        arrs = {n.replace("/", "__"): get(n) for n in self.keras_shapes}
        with open(path, "wb") as f:
            np.savez(f, **arrs)

    def load_weights(self, path, by_name=True, skip_mismatch=False, name_map=None):
        """model.load_weights(path, by_name=True, skip_mismatch=True) -- eval.py:140.  Reads ``.npz`` (this library) and
        Keras ``.h5`` weight files (h5lite: contiguous float datasets, old-style groups -- what Keras / h5py write).
        Weights are matched BY NAME: ``<layer>/<weight>`` of ``model.layers_spec``; ``name_map`` ({file layer name: model
        layer name}) renames layers of a file whose auto-generated Keras names differ (the reference's checkpoints are
        not available here, so their exact layer names are unpinned).  Unknown layers are ignored (by_name semantics);
        a shape mismatch raises unless ``skip_mismatch``."""
        path = str(path)
        name_map = name_map or {}
        items = []
        if path.endswith((".h5", ".hdf5")):
            from . import h5lite
            _, layers = h5lite.read_keras_weights(path)
            for ln, ws in layers.items():
                tgt = name_map.get(ln, ln)
                for wn, arr in ws:
                    w = wn.split("/")[-1].split(":")[0]
                    items.append((f"{tgt}/{w}", arr))
        else:
            with np.load(path, allow_pickle=False) as z:
                items = [(name_map.get(k.replace("__", "/"), k.replace("__", "/")), z[k]) for k in z.files]
        for n, arr in items:
            if n not in self.keras_shapes:
                continue
            if tuple(arr.shape) != tuple(self.keras_shapes[n]):
                if skip_mismatch:
                    continue
                raise ValueError(f"shape mismatch for {n}: {arr.shape} vs {self.keras_shapes[n]}")
            self.set_weight(n, arr)

    def count_params(self):
        return int(sum(np.prod(s) for s in self.keras_shapes.values()))

    def summary(self, print_fn=print):
        print_fn(f'Model: "{type(self).__name__}"')
        for layer, ws in self.layers_spec.items():
            n = sum(int(np.prod(self.keras_shapes[f"{layer}/{w}"])) for w in ws)
            print_fn(f"  {layer:36s} {n:>12,d}")
        print_fn(f"Total params: {self.count_params():,d}")
        size = lambda names: int(sum(np.prod(self.keras_shapes[n]) for n in names))
        print_fn(f"Trainable params: {size(self.trainable_names()):,d}")
        print_fn(f"Non-trainable params: {size(self.non_trainable_names()):,d}")

    # ------------------------------------------------------------------ input corruption (scan_dropout=, word_dropout=)
    SUPPORTS_INPUT_CORRUPTION = False   # True on nic.NIC and lc_nic.NIC, whose train_step stages with corrupt=True
    def _input_width(self):
        """the voxel columns of a staged scan row (lc_nic.NIC: n_in)"""
        return self.N

    @property
    def scan_dropout(self):
        """the model's model_base.ScanDropout, or None; assignable (validated), and a new rate needs no re-recording: the
        launch sits with the staging, outside the recorded step"""
        return self._scan_dropout

    @scan_dropout.setter
    def scan_dropout(self, sd):
        if sd is not None and not isinstance(sd, ScanDropout):
            raise ValueError(f"scan_dropout must be None or a model_base.ScanDropout, got {sd!r}")
        if sd is not None and not self.SUPPORTS_INPUT_CORRUPTION:
            raise NotImplementedError(f"{type(self).__name__} has no scan_dropout: it is built for nic.NIC and lc_nic.NIC")
        if sd is not None and sd.null is not None and sd.null.shape[0] != self._input_width():
            raise ValueError(f"the null scan of scan_dropout must have the model's input width {self._input_width()}, "
                             f"got {sd.null.shape[0]}")
        compat.check(self, ("corruption",), _scan_dropout=sd)
        self._scan_dropout = sd
        self._null_dev = None if sd is None or sd.null is None else torch.from_numpy(sd.null.copy()).to(self.device)

    @property
    def word_dropout(self):
        """the model's model_base.WordDropout, or None; assignable (validated), without re-recording"""
        return self._word_dropout

    @word_dropout.setter
    def word_dropout(self, wd):
        if wd is not None and not isinstance(wd, WordDropout):
            raise ValueError(f"word_dropout must be None or a model_base.WordDropout, got {wd!r}")
        if wd is not None and not self.SUPPORTS_INPUT_CORRUPTION:
            raise NotImplementedError(f"{type(self).__name__} has no word_dropout: it is built for nic.NIC and lc_nic.NIC")
        if wd is not None and wd.unk_id >= self.V:
            raise ValueError(f"word dropout unk_id {wd.unk_id} is not below vocab_size {self.V}")
        compat.check(self, ("corruption",), _word_dropout=wd)
        self._word_dropout = wd

    @property
    def null_scan(self):
        """the (N,) float32 null scan of the model's ScanDropout (whatever its rate: no decode corrupts its input), or None;
        ``guidance=Guidance(scale, null=None)`` decodes against it"""
        sd = self._scan_dropout
        return None if sd is None or sd.null is None else sd.null

    def _corruption(self, pending=None):
        """(ScanDropout or None, WordDropout or None) with a neutral one as None, or None when neither is active: then the
        step issues the launches it issues without the keywords.  ``pending``: as _token_weights_on takes it"""
        sd, wd = self._scan_dropout, self._word_dropout
        if pending:
            sd, wd = pending.get("_scan_dropout", sd), pending.get("_word_dropout", wd)
        sd = None if sd is None or sd.neutral else sd
        wd = None if wd is None or wd.neutral else wd
        return (sd, wd) if (sd is not None or wd is not None) else None

    def _corrupt_check(self):
        """what a model with active input corruption refuses, as it stands (compat.check on ``corruption``)"""
        compat.check(self, ("corruption",))

    def _input_corrupt(self, cor, B, T, n_cols):
        """tnt_input_corrupt_f32 on the staged x (and its voxel-major copy) and cap, at this step's drop_step: one launch
        directly behind the staging, outside the recorded step"""
        sd, wd = cor
        xT = self.xT if sd is not None else None
        self.be.input_corrupt(self.x if sd is not None else None, self.ldx, xT, xT.shape[1] if xT is not None else 0,
                              self.cap if wd is not None else None, B, T, n_cols, self.V,
                              sd.rate if sd is not None else 0.0, self._null_dev if sd is not None else None,
                              wd.rate if wd is not None else 0.0, wd.unk_id if wd is not None else 0,
                              self.seed, S_SCAN_DROP, S_WORD_DROP, self.drop_step)

    # ------------------------------------------------------------------ input staging
    def _to_dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype, non_blocking=True)
        return torch.as_tensor(np.asarray(a), dtype=dtype).to(self.device, non_blocking=True)

    def _stage_mask_job(self):
        """(out, n, nsites, rate, seed, site0, step_dev) of the dropout masks a training step wants generated with its
        batch staging (attention model: the stored attention-dropout masks of all T steps), or None"""
        return None

    def _head_map_bufs(self, B, T):
        """(pos, row_weight, tgt_compact, live, loss_row, corr_row) when this model wants the vocabulary head's row map built
        with the staging of a training batch (nic.NIC: compact_head), else None"""
        return None

    def _stage_fwd_args(self, B):
        """(w, part, gx_part, w2_part, E, ldw, nsplit) when the model's training forward begins with the streaming encoder
        product of the staged batch and wants it in the staging launch (nic.NIC: stage_fwd), else None"""
        return None

    def _stage_batch(self, inputs, target, n_cols, masks=False, head_map=False, fwd=False, corrupt=False):
        """(inputs, target) -> static buffers.  A batch that already sits on the model's device in the staged
        dtypes (float32 -- or float16 "on-wire" -- betas, float32 states, int32 ids, contiguous) goes through ONE launch
        (tnt_stage_batch_f32 / _h16);
        anything else (numpy, one-hot targets, other dtypes) takes the general per-tensor path.
        ``corrupt`` (the training steps): behind whichever route ran, the model's scan / word dropout as one launch on the
        staged buffers (_input_corrupt); a model without them, or with neutral ones, issues nothing."""
        cor = self._corruption() if corrupt else None
        x, cap, a0, c0 = inputs[:4]
        if target is not None and self.unlikelihood > 0 and np.shape(cap)[-1] > self.UNLIKELIHOOD_MAX_T:
            # a step with a loss: refused here, in front of every launch (and so outside any capture)
            raise ValueError(f"unlikelihood training holds a caption's prefix in one wave: at most {self.UNLIKELIHOOD_MAX_T} "
                             f"loss positions per caption, got {np.shape(cap)[-1]}")
        ts = [x, cap, a0, c0] + ([target] if target is not None else [])
        dev = self.device
        same = lambda t: t.device.type == dev.type and (t.device.index or 0) == (dev.index or 0)
        ok = all(isinstance(t, torch.Tensor) and same(t) and t.is_contiguous() for t in ts)
        ok = ok and x.dtype in (torch.float32, torch.float16) and a0.dtype == c0.dtype == torch.float32
        ok = ok and cap.dtype == torch.int32
        ok = ok and x.dim() == 2 and cap.dim() == 2 and x.shape == (cap.shape[0], n_cols)
        ok = ok and (target is None or (target.dtype == torch.int32 and target.shape == cap.shape))
        route = self._route = StepRoute()        # a new batch: nothing is handed over from the step before
        if not ok:
            B, T = self._stage_inputs(inputs)
            route = self._route                 # (_stage_inputs stages a batch too)
            if target is not None:
                self._stage_target(target, B, T)
            mk = self._stage_mask_job() if masks else None
            if mk is not None:
                self.be.dropout_mask4(mk[0], mk[1], mk[2], mk[3], mk[4], mk[5], 0, mk[6])
            route.masks_staged = mk is not None
            if cor is not None:
                self._input_corrupt(cor, B, T, n_cols)
            return B, T
        B, T = cap.shape
        self._build(B, T)
        assert a0.shape == c0.shape == (B, self.U), f"state shape {tuple(a0.shape)} != {(B, self.U)}"
        xT = self.xT                        # voxel-major copy for the region-wise encoder, written in the same launch
        kw = {}
        mk = self._stage_mask_job() if masks else None
        if mk is not None:                   # the step's dropout masks ride in the staging launch
            kw["masks"] = mk
        route.masks_staged = mk is not None
        hm = self._head_map_bufs(B, T) if (head_map and target is not None and mk is None and xT is None
                                           and x.dtype == torch.float32) else None
        # scan dropout declines the stage_fwd ride: the encoder forward inside that launch reads the caller's x in place,
        # not the staged rows the corruption writes (word dropout keeps it: the row map merges on id 0 only)
        sf = self._stage_fwd_args(B) if (fwd and hm is not None and n_cols == self.ldx
                                         and (cor is None or cor[0] is None)) else None
        if sf is not None and self.be.dense_fwd_stream_gram_stage(x, *sf[:4], B, sf[4], n_cols, sf[5], sf[6], self.x, self.ldx,
                                                                  cap, self.cap, target, self.tgt, a0, self.Hs[0], c0,
                                                                  self.Cs[0], T, self.U, *hm):
            # ... and both ride behind the encoder forward, which reads the caller's x in place: the step's first launch is
            # the forward, and _forward leaves its own out (False: the entry refused these arguments, e.g. their alignment)
            route.head_map_fresh = route.stage_fwd_done = True
        elif hm is not None:
            # the head's row map (which caption positions repeat an earlier row) rides in the staging launch: the step that
            # follows runs its vocabulary head over the distinct rows only
            self.be.stage_batch_map(x, self.x, cap, self.cap, target, self.tgt, a0, self.Hs[0], c0, self.Cs[0], B, T, n_cols,
                                    self.ldx, self.U, *hm)
            route.head_map_fresh = True
        elif xT is not None:
            self.be.stage_batch(x, self.x, cap, self.cap, target, self.tgt, a0, self.Hs[0], c0, self.Cs[0], B, T, n_cols,
                                self.ldx, self.U, xT, xT.shape[1], **kw)
        else:
            self.be.stage_batch(x, self.x, cap, self.cap, target, self.tgt, a0, self.Hs[0], c0, self.Cs[0], B, T, n_cols,
                                self.ldx, self.U, **kw)
        if cor is not None:
            self._input_corrupt(cor, B, T, n_cols)
        return B, T

    def _stage_target(self, target, B, T):
        """target: one-hot (B,T,V) float (to_categorical, data_generator_guse.py:163) or int ids (B,T).
        Fills self.tgt (time-major int32 ids)."""
        if isinstance(target, np.ndarray) and target.ndim == 2 or (isinstance(target, torch.Tensor) and target.dim() == 2):
            t = self._to_dev(target, torch.int32)
            self.tgt.view(T, B).copy_(t.t())
        else:
            oh = self._to_dev(target, torch.float32).contiguous()
            assert oh.shape == (B, T, self.V), f"target shape {tuple(oh.shape)}"
            self.be.onehot_argmax(oh, self.tgt, B, T, self.V)

    # ------------------------------------------------------------------ device guard (persistent LSTM kernel)
    def _guard_word(self):
        """The error word of the persistent kernel's sync state (uint32, device) while that kernel is in use, else None.
        The optimizer kernels take it as ``guard`` and leave the model untouched when it is set."""
        sync = self.seq_sync
        return sync[1024:1025] if (sync is not None and self._seq_lstm) else None

    def _guard_out(self):
        """Where the persistent kernel reports its error code for the host: slot GUARD of the metrics buffer."""
        return self.met[self.GUARD:self.GUARD + 1]

    def _seq_chain(self, bwd=False):
        """The ``chain`` argument of lstm_layer_fwd / lstm_layer_bwd (``bwd``: with the BPTT's exchange buffer) while the
        persistent kernel is in use, else None: the per-step kernels."""
        if not self._seq_lstm or (bwd and self.seq_xch is None):
            return None
        return (self.seq_sync, self._guard_out()) + ((self.seq_xch,) if bwd else ())

    def _run_step(self, run, key, fn):
        """``run(key, fn)`` (_run_captured / _run_planned) for a training step; returns whether that step's finalize launch
        filed the metrics vector in the ring (known when ``fn`` actually runs -- eager or under capture --, remembered per
        key for the replays)."""
        graphs = self.use_graph and self.device.type == "cuda"
        st = self._graphs.get(key) if graphs else None
        executed = (not graphs) or st is None or (isinstance(st, str) and st == "warm")
        self._ring_hit = False
        run(key, fn)
        keys = self._ring_keys
        if executed or self._ring_hit:
            (keys.add if self._ring_hit else keys.discard)(key)
        return key in keys

    def _met_snapshot(self, ring=False):
        """This step's metrics vector: the row the step's Adam launch copied it to (``ring``: fused single-process step, no
        device copy behind the step -- a 5 us launch on a 0.55 ms step), else a clone of ``met``."""
        if ring:
            t = self._ring_host
            self._ring_host = t + 1
            row = self.met_ring[t % self.METRIC_RING]
            self._last_ring = (row, t & 0xFFFFFF)
            return row
        self._last_ring = None
        return self.met.clone()

    def _ring_args(self):
        """keyword arguments that make the Adam launch of the fused step file the metrics vector in the ring"""
        if not self.metric_ring or self.met is None or self.met.numel() > 62:
            return {}
        if self.met_ring is None or self.met_ring.shape[1] != self.met.numel() + 1:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                return {}
            self.met_ring = self._f(self.METRIC_RING, self.met.numel() + 1)
            self.ring_t = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ring_host = 0
            self._graphs = {}
        self._ring_hit = True
        return dict(met=self.met, ring=self.met_ring, ring_t=self.ring_t)

    def _metrics_from(self, m, **slots):
        """Metrics from a snapshot ``m`` of the metrics buffer (_met_snapshot); the guard word of the same snapshot rides along."""
        out = Metrics((k, m[i] if isinstance(i, int) else i) for k, i in slots.items())
        out._ring = self._last_ring
        return out.guarded(self, m[self.GUARD]) if self._seq_lstm else out

    def _on_guard_trip(self, code):
        self.disable_seq_lstm()
        what = {1: "a barrier timed out", 2: "a launch did not place 32 workgroups on every XCD"}.get(code, "unknown")
        accum = ""
        if self._accum_host is not None:
            # the faulted micro-step left the accumulator alone, but its place in the window is lost: start the window again
            self._accum_j = 0
            accum = ("  Gradient accumulation: the open window was dropped -- its earlier micro-batches were discarded, the "
                     "next train_step opens a new window.")
        raise DeviceGuardError(
            f"persistent LSTM kernel: device guard tripped (code {code}: {what}).  The results of that step are invalid; "
            "its optimizer update was skipped, so weights, moments and step counters are unchanged.  NOT unchanged: the "
            "BatchNorm moving mean / variance, which the forward pass of the faulted step already advanced (a retried step "
            "applies that 1 % moving-average update a second time), and under data parallel the trip is per rank -- the other "
            "replicas have applied their update, so re-broadcast the parameters (dp.broadcast_parameters) before going on.  "
            "The model now uses the per-step LSTM kernels: run the step again." + accum)

    def _guarded(self, fn):
        """Inference paths: run ``fn`` (which ends in a host read anyway), check the guard word, and on a trip fall back
        to the per-step kernels and run it once more -- inference mutates no model state."""
        out = fn()
        if self._guard_word() is not None and float(self.met[self.GUARD]) != 0.0:
            self.disable_seq_lstm()
            out = fn()
        return out

    def check_device_errors(self):
        """Raises DeviceGuardError if the persistent LSTM kernel's error word is set (synchronises).  train_step /
        test_step results carry the same check with them (Metrics.as_floats), the inference paths check after their
        own host read; this is the explicit form for loops that never read a metric."""
        sync = self.seq_sync
        if sync is not None and int(sync[1024].item()) != 0:
            self._on_guard_trip(int(sync[1024].item()))

    def _init_seq_lstm(self, B, U):
        """Opt in to the persistent sequence-forward kernel for this (B, U) on this device.  Probes once per process
        (tnt_lstm_seq_supported synchronises), so it is called from _build, outside any capture."""
        self._seq_lstm = bool(self.use_seq_lstm and hasattr(self.be, "lstm_seq_supported")
                              and self.be.lstm_seq_supported(B, U))
        if self._seq_lstm and self.seq_sync is None:
            self.seq_sync = torch.zeros(1025, dtype=torch.int32, device=self.device)     # re-armed by the kernel itself
        if self._seq_lstm and hasattr(self.be, "lstm_seq_bwd"):
            n = self.be.lstm_seq_bwd_work_floats(B, U)       # exchange buffer of the persistent BPTT chain
            if self.seq_xch is None or self.seq_xch.numel() < n:
                self.seq_xch = self._f(n)
        else:
            self.seq_xch = None

    def disable_seq_lstm(self):
        """Back to the per-step LSTM kernels (after a guard trip of the persistent one, or by choice): zeroes the sync
        state and the guard slot, drops captured graphs / launch plans; the step buffers are reused as they are."""
        self.use_seq_lstm = False
        sync = self.seq_sync
        if sync is not None:
            sync.zero_()
        if self.met is not None:
            self.met[self.GUARD] = 0
        self._seq_lstm = False
        self._graphs = {}

    # ------------------------------------------------------------------ graph capture
    def _sample_step_word(self, step):
        """the static device word a captured sampled decode reads its Philox stream step from (step_dev), set to
        ``step`` (mod 2^32) on the stream before the launch or replay"""
        w = self._step_word
        if w is None:
            w = self._step_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        w.fill_(int(np.uint32(int(step) & 0xFFFFFFFF).view(np.int32)))
        return w

    def _decode_bufs(self, name):
        """the buffer dict ``name`` (_con_bufs / _cons_bufs / _mbr_bufs), made on first use"""
        if getattr(self, name) is None:
            setattr(self, name, {})
        return getattr(self, name)

    def _constrain(self, constraints, rows, max_len, beam_width=1, end_id=-1):
        """The constrained-decode helper of a decode over ``rows`` rows (``end_id``: beam search's), or None when
        ``constraints`` is None or neutral: then the decode issues no new launch and keeps its capture key and buffers.
        Refusals (ValueError, before any launch): max_len > 64; a bad id outside [0, V); min_length without an end_id >= 1
        or above max_len; two different end ids; and len(bad_ids) + max_len + 1 + beam_width > V, so that every live row
        keeps at least beam_width tokens un-banned at every step."""
        c = constraints
        if c is None:
            return None
        if not isinstance(c, DecodeConstraints):
            raise ValueError(f"constraints must be a DecodeConstraints or None, got {c!r}")
        if c.neutral:
            return None
        V = self.V
        if max_len > c.MAX_LEN:
            raise ValueError(f"constrained decoding holds at most {c.MAX_LEN} tokens per caption, got max_len = {max_len}")
        if any(v >= V for v in c.bad_ids):
            raise ValueError(f"bad_ids must be token ids in [0, {V}), got {c.bad_ids}")
        if c.end_id >= 0 and end_id >= 0 and c.end_id != end_id:
            raise ValueError(f"constraints.end_id = {c.end_id} differs from the decode's end_id = {end_id}")
        eid = c.end_id if c.end_id >= 0 else int(end_id)
        if c.min_length > 0 and not 1 <= eid < V:
            raise ValueError(f"min_length = {c.min_length} needs an end_id in [1, {V}), got {eid}")
        if c.min_length > max_len:
            raise ValueError(f"min_length = {c.min_length} exceeds max_len = {max_len}")
        if len(c.bad_ids) + max_len + 1 + beam_width > V:
            raise ValueError(f"{len(c.bad_ids)} bad ids + max_len {max_len} + 1 + beam width {beam_width} exceed the "
                             f"vocabulary of {V}: a step could be left without a token to choose")
        return _ConstrainedDecode(self, c, rows, max_len, eid if c.min_length > 0 else -1)

    def _consensus(self, consensus, img_input, n_start, beam_width=1, training=False):
        """The consensus-decode helper (``img_input``: the scans to stage, ``n_start`` entries of start_seq), or None when
        ``consensus`` is None: then the decode issues the launches it issues without the keyword, under the same capture
        key.  Refusals (before any launch): not a Consensus; training=True; a data-parallel model; n_rows not G * n_start;
        for a multi-subject model, members other than n_subjects (the subject slices are the members)."""
        c = consensus
        if c is None:
            return None
        if not isinstance(c, Consensus):
            raise ValueError(f"consensus must be a Consensus or None, got {c!r}")
        if training:
            raise ValueError("consensus decoding is an inference mode: training=True is refused")
        if self.grad_sync is not None:
            raise NotImplementedError("consensus decoding has no data-parallel schedule: decode on one device")
        G, S = c.members, int(self.S)
        n_rows = int(img_input.shape[0]) if hasattr(img_input, "shape") else len(img_input)
        if S > 1 and G != S:
            raise ValueError(f"a model of n_subjects = {S} decodes the consensus of its subject slices: members must be {S}, "
                             f"got {G}")
        if n_rows % G:
            raise ValueError(f"consensus of {G} members needs G * M input rows (member-major), got {n_rows}")
        if n_rows != G * n_start:
            raise ValueError(f"consensus of {G} members over {n_rows} input rows decodes {n_rows // G} captions: start_seq "
                             f"must have {n_rows // G} entries, got {n_start}")
        return _ConsensusDecode(self, c, n_start, int(beam_width))

    def _guidance(self, guidance, img_input, a0, c0, n_start, beam_width=1, consensus=None, diversity=None, training=False):
        """The guided-decode helper and the inputs it decodes, ``(helper, img_input, a0, c0)`` with the 2 * M rows
        member-major (the scans, then their null scans; a0 / c0 repeated), or None when ``guidance`` is None or neutral:
        then the decode issues the launches it issues without the keyword, under the same capture key.  Refusals (before
        any launch): not a Guidance; together with consensus or diverse beams; training=True; a data-parallel model;
        n_subjects > 1; img_input rows other than n_start; a null scan whose shape does not fit the batch."""
        g = guidance
        if g is None:
            return None
        if not isinstance(g, Guidance):
            raise ValueError(f"guidance must be a Guidance or None, got {g!r}")
        if g.neutral:
            return None
        if consensus is not None:
            raise ValueError("guidance together with consensus is not supported: pass one of the two")
        if diversity is not None:
            raise ValueError("guidance together with diversity (diverse beam search) is not supported: pass one of the two")
        if training:
            raise ValueError("guided decoding is an inference mode: training=True is refused")
        if self.grad_sync is not None:
            raise NotImplementedError("guided decoding has no data-parallel schedule: decode on one device")
        S = int(self.S)
        if S > 1:
            raise ValueError(f"guided decoding is built for one subject: n_subjects = {S} is not supported")
        if not hasattr(img_input, "shape"):
            img_input = np.asarray(img_input)
        shape = tuple(int(v) for v in img_input.shape)
        if len(shape) != 2 or shape[0] != n_start:
            raise ValueError(f"guided decoding takes one scan per caption: img_input must be ({n_start}, N) for the "
                             f"{n_start} entries of start_seq, got {shape}")
        null = g.null if g.null is not None else self.null_scan        # (a ScanDropout model: the null it was trained on)
        if null is None:
            null = np.zeros(shape[1], np.float32)
        if null.shape != shape[1:] and null.shape != shape:
            raise ValueError(f"the null scan must have shape {shape[1:]} or {shape} for this batch, got {null.shape}")
        null = np.ascontiguousarray(np.broadcast_to(null, shape))

        def twice(t, second=None):
            if isinstance(t, torch.Tensor):
                u = t if second is None else torch.as_tensor(second).to(device=t.device, dtype=t.dtype)
                return torch.cat([t, u], dim=0)
            t = np.asarray(t)
            return np.concatenate([t, t if second is None else second.astype(t.dtype)], axis=0)
        return _GuidanceDecode(self, g, n_start, int(beam_width)), twice(img_input, null), twice(a0), twice(c0)

    def _diversity(self, diversity, beam_width):
        """(groups, penalty) of a diverse beam search (check_diversity), or None when ``diversity`` is None or has one
        group: then the search issues the launches it issues without the keyword, under the same capture key.  Refusals
        (before any launch): not a BeamDiversity; groups that do not divide beam_width; a data-parallel model."""
        div = check_diversity(diversity, int(beam_width))
        if div is not None and self.grad_sync is not None:
            raise NotImplementedError("diverse beam search has no data-parallel schedule: decode on one device")
        return div

    def _decode_setup(self, guidance, consensus, constraints, diversity, img_input, a0, c0, start_seq, max_len, beam_width=1,
                      end_id=-1, training=False):
        """What greedy_predict, sample_predict and beam_search resolve in front of their loops, in the order that decides
        which refusal a bad call gets: the start tokens, ``diversity``, ``guidance`` before ``consensus``, ``training``,
        then ``constraints`` over the decoder's row count.  Returns (cons, (img_input, a0, c0), start, M, G, B, con, div,
        ckey): the member helper (_GuidanceDecode or _ConsensusDecode) or None; the inputs to stage (doubled under
        guidance); the start tokens on the device, repeated per member (B,); M captions from G members' B = G * M staged
        scans (the decoder runs B * beam_width rows, member-major); the constraint helper over those rows or None;
        (groups, penalty) or None; and the suffix the keywords add to the capture key."""
        k = beam_width
        start = self._to_dev(np.asarray(start_seq).reshape(-1), torch.int32)
        M = start.shape[0]
        div = self._diversity(diversity, k)
        guide = self._guidance(guidance, img_input, a0, c0, M, k, consensus, div, training)
        if guide is not None:
            cons, img_input, a0, c0 = guide
        else:
            cons = self._consensus(consensus, img_input, M, k, training)
        assert training is False, "training is set to True"                                  # lc_NIC.py:591
        G = cons.G if cons is not None else 1
        B = G * M
        con = self._constrain(constraints, B * k, max_len, k, int(end_id))
        ckey = ((con.key if con is not None else ()) + (cons.key if cons is not None else ())
                + (("diverse",) + div if div is not None else ()))
        return cons, (img_input, a0, c0), start.repeat(G) if cons is not None else start, M, G, B, con, div, ckey

    def _run_captured(self, key, fn):
        """Run ``fn`` (a fixed launch sequence over static buffers) through a hipGraph:
        first call eager (warm-up), second call captures, later calls replay."""
        if not (self.use_graph and self.device.type == "cuda"):
            fn()
            return
        st = self._graphs.get(key)
        if st is None:
            fn()
            self._graphs[key] = "warm"
        elif st == "warm":
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog thread may query events while we capture (data parallel)
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                fn()
            self._graphs[key] = g
            g.replay()
        else:
            st.replay()

    def _run_planned(self, key, fn):
        """Like _run_captured, but the segment is replayed as a recorded list of C-ABI launches instead of a
        hipGraph: first call eager, second call records every backend call ``fn`` makes (HipBackend._call), later
        calls re-issue those bound calls.  The device sees plain kernel launches -- no graph-launch gap (~15-20 us
        per hipGraphLaunch) -- and the host skips the Python argument plumbing (~9 -> ~4 us per launch).  Same
        contract as capture: ``fn`` may only make backend launches on static buffers, on the current stream."""
        if not (self.use_graph and self.device.type == "cuda"):
            fn()
            return
        st = self._graphs.get(key)
        if st is None:
            fn()
            self._graphs[key] = "warm"
            return
        stream = self.be._s()
        if st == "warm" or st[0] != stream:
            self.be._rec = rec = []
            try:
                fn()
            finally:
                self.be._rec = None
            self._graphs[key] = (stream, rec)
            return
        for f, name, args in st[1]:
            if f(*args) != 0:
                raise RuntimeError(f"{name} failed while replaying launch plan {key}")

    # ------------------------------------------------------------------ training-step scaffold (the model supplies _train_graph)
    def _update_graph(self):
        self._apply_agc()
        self._norms_and_l2(self.met[2:3])
        self._apply_optimizer()

    def _train_and_update_graph(self, B, T):
        """the single-process step as one launch sequence: the loss / accuracy totals ride in the step-finalize launch"""
        if not self.fused_update:          # A/B switch (tools/ab_attr.py): the unfused launch sequence
            self._train_graph(B, T)
            self._update_graph()
            return
        with self._deferring():
            self._train_graph(B, T)
        self._update_fused(self.met[2:3])

    @contextmanager
    def _deferring(self, on=True):
        """The scope of a step's launches that may leave work to the fused update behind them (StepTail): _sum2,
        _embedding_bwd and the models' _loss_metrics / _bwd_enc read ``_tail.deferring``.  It opens on an empty tail, so
        nothing is inherited from an earlier step that failed between its loss and its update; what the scope collects
        stays for the _update_fused that follows.  ``on=False``: the same launches with nothing deferred."""
        self._tail = StepTail(deferring=bool(on))
        try:
            yield
        finally:
            self._tail.deferring = False

    def _train_step_dp(self, B, T, fb, up):
        """the generic data-parallel schedule: forward+backward | all-reduce of the flat gradient | update"""
        self._run_captured(("train_fb", B, T), fb)
        self.grad_sync(self)
        self._run_captured(("train_up", B, T), up)

    # The single-process step is replayed as a recorded launch plan (_run_planned), not as a hipGraph: with 15 (dense) / 32
    # (attention) launches a step the host re-issues them in ~15 % of the step's time and every launch starts ~0.2-0.4 us
    # earlier than as a graph node (0.4650 -> 0.4588 and 0.5666 -> 0.5626 ms/step, tools/probe/plan_bench.py: separate
    # models, repeated, spread 0.0005).  ``plan_step = False`` restores the graph.  A plan re-issues backend launches
    # only, so it is used where the step is nothing else: the sparse Embedding backward (the dense form hands its ids on
    # with a tensor copy, which a graph captures and a plan would drop).
    def _step_runner(self, E=None):
        """_run_planned where the training step is backend launches only, else _run_captured.  ``E``: the text-embedding
        width (default self.E)"""
        plan = self.plan_step and (self.E if E is None else E) % 4 == 0 and self.sparse_emb_bwd
        return self._run_planned if plan else self._run_captured

    def _ss_refuse(self, T):
        """behind the staging of a scheduled-sampling train_step (``T``: the staged caption length): a caption with more
        token positions than the Philox sites hold"""
        if self.scheduled_sampling is not None and T - 1 > SS_MAX_POSITIONS:
            raise ValueError(f"scheduled sampling decides at most {SS_MAX_POSITIONS} token positions per caption "
                             f"(Philox sites S_SS_COIN/S_SS_DRAW + j): caption length {T} is too long")

    def _probs(self, B, T):
        """softmax over the logits in place (one launch); returns the probabilities as (B, T, V)"""
        self.be.softmax_cce(self.logits, None, self.logits, None, None, None, T * B, self.V, self.ldV, 0.0)
        return self.logits.view(T, B, self.ldV)[:, :, :self.V].permute(1, 0, 2).contiguous()

    def _sam_move(self, rho, phase, sq_override=None):
        """the weight move of a sharpness-aware step (tnt_sam_f32): phase 0 steps to theta + rho * g / ||g|| and keeps the
        offset in ``ew``, phase 1 steps back"""
        a, sp = self.arena, self.arena.spans
        self.be.sam(a.theta, a.grad, self.ew, sp.span_seg, sp.span_off, sp.span_len, a.seg_l2, a.sq, a.nseg, sp.nspan, rho, phase,
                    sq_override=sq_override)

    # ------------------------------------------------------------------ caption scoring
    def score_captions(self, img_input, a0, c0, captions, end_id=-1, normalise=None, return_tokens=False, max_rows=None):
        """log p(caption | scan) under the teacher-forced inference forward (definition: tnt_caption_score_f32 in
        include/tnt_hip.h).  captions: int (B, T), row b the caption of scan b exactly as train_step takes it (column 0 the
        start token) -> (logprob (B,) float32, length (B,) int32); or int (B, C, T), C candidate captions per scan ->
        (logprob (B, C), length (B, C)).  A position counts up to and including the first ``end_id`` (-1: none) and never
        at or behind a 0; length is the number of counted positions.  ``normalise``: None = the sum, "mean" = the sum
        / max(length, 1).  ``return_tokens``: also tok_lp (B, [C,] T-1), 0 at positions that do not count.

        The encoder runs on the B scans once per call; its result is gathered to the B*C decoder rows on the device (row
        b*C + c).  ``max_rows`` bounds the decoder rows of one pass: the candidates are processed in chunks of
        max_rows // B whole candidates over buffers sized for one chunk.  Default: as many whole candidates as keep one
        pass's logits ((T-1) * ld(V) * 4 bytes per decoder row) within SCORE_LOGITS_BYTES = 256 MiB, at least one.  Each
        pass is one recorded sequence per (B, chunk, T, end_id), replayed like greedy_predict; the captions reach it
        through a device buffer, and the results (with the persistent chain's guard word) come back in one copy.
        The model's weights, optimizer state and Philox counters are not touched."""
        if normalise not in (None, "mean"):
            raise ValueError(f"normalise must be None or 'mean', got {normalise!r}")
        caps = captions.detach().cpu().numpy() if isinstance(captions, torch.Tensor) else np.asarray(captions)
        if caps.ndim not in (2, 3) or not np.issubdtype(caps.dtype, np.integer):
            raise ValueError(f"captions must be an integer array (B, T) or (B, C, T), got {caps.dtype} {caps.shape}")
        flat = caps.ndim == 2
        caps = np.ascontiguousarray(caps[:, None, :] if flat else caps, dtype=np.int32)
        B, C, T = caps.shape
        if B < 1 or C < 1 or T < 2:
            raise ValueError(f"captions {caps.shape}: need at least one scan, one candidate and two positions")
        end_id = int(end_id)
        if end_id >= self.V or end_id < -1 or end_id == 0:
            raise ValueError(f"end_id must be -1 (none) or a token id in [1, {self.V}), got {end_id}")
        self._score_refuse()
        steps = T - 1
        if max_rows is None:
            max_rows = max(1, SCORE_LOGITS_BYTES // (steps * self.ldV * 4) // B) * B
        max_rows = int(max_rows)
        if max_rows < B:
            raise ValueError(f"max_rows = {max_rows} is below the batch of {B} scans: one pass holds at least one candidate "
                             "per scan")
        Cc = min(C, max_rows // B)
        self._stage_inputs((img_input, caps[:, 0, :], a0, c0))          # the B scans, their state; builds the (B, T) buffers
        n = B * C

        def run():
            st = self._score_state(B, Cc, C, T)
            st["caps"].copy_(torch.from_numpy(caps), non_blocking=True)
            res = st["res"]
            lp_all, len_all = res[:n].view(B, C), res[n:2 * n].view(torch.int32).view(B, C)
            tok_all = res[2 * n + 1:].view(B, C, steps)
            for c_lo in range(0, C, Cc):
                Cr = min(Cc, C - c_lo)
                v = self._score_views(st, B, Cr, T)
                v["cap"].view(B, Cr, T).copy_(st["caps"][:, c_lo:c_lo + Cr])
                first = c_lo == 0
                self._run_captured(("score", B, Cr, T, end_id, first), lambda: self._score_pass(B, Cr, T, end_id, v, first))
                lp_all[:, c_lo:c_lo + Cr].copy_(v["cap_lp"].view(B, Cr))
                len_all[:, c_lo:c_lo + Cr].copy_(v["cap_len"].view(B, Cr))
                if return_tokens:
                    tok_all[:, c_lo:c_lo + Cr].copy_(v["tok_lp"].view(steps, B, Cr).permute(1, 2, 0))
            guard = self._guard_word() is not None
            if guard:
                res[2 * n:2 * n + 1].copy_(self.met[self.GUARD:self.GUARD + 1])
            host = (res if return_tokens else res[:2 * n + 1]).cpu().numpy()         # the call's one device-to-host copy
            return host, guard and host[2 * n] != 0.0
        host, tripped = run()
        if tripped:                  # as _guarded: fall back to the per-step kernels and run once more
            self.disable_seq_lstm()
            host, _ = run()
        lp = host[:n].reshape(B, C).copy()
        length = host[n:2 * n].view(np.int32).reshape(B, C).copy()
        if normalise == "mean":
            lp = lp / np.maximum(length, 1).astype(np.float32)
        out = (lp[:, 0], length[:, 0]) if flat else (lp, length)
        if return_tokens:
            tok = host[2 * n + 1:].reshape(B, C, steps).copy()
            out += (tok[:, 0] if flat else tok,)
        return out

    def _score_refuse(self):
        raise NotImplementedError(f"{type(self).__name__} has no caption scoring")

    def _score_state(self, B, Cc, C, T):
        """per (B, chunk, C, T): the captions (B, C, T) on the device, the packed results [logprob B*C | length B*C (int32
        bits) | guard word | tok_lp B*C*(T-1)], and the model's decoder buffers for one chunk of B*Cc rows (_score_bufs),
        allocated once and viewed per pass (_score_views)"""
        st = self._score
        key = (B, Cc, C, T, bool(self._seq_lstm))
        if st is None or st["key"] != key:
            n = B * C
            st = self._score = dict(key=key, caps=torch.zeros(B, C, T, dtype=torch.int32, device=self.device),
                                    res=self._f(2 * n + 1 + n * (T - 1)), views={})
            st.update(self._score_bufs(B * Cc, T))
            for k in [k for k in self._graphs if isinstance(k, tuple) and k and k[0] == "score"]:
                del self._graphs[k]             # recorded over the buffers just replaced
        return st

    def _score_views(self, st, B, Cr, T):
        """the chunk buffers viewed for a pass of R = B*Cr rows (the prefix of each allocation: same addresses every call),
        and the gather index of the pass (decoder row b*Cr + c <- scan b)"""
        v = st["views"].get(Cr)
        if v is None:
            R = B * Cr
            v = st["views"][Cr] = self._score_shape(st, R, T)
            v["rep"] = torch.arange(B, dtype=torch.int32, device=self.device).repeat_interleave(Cr).view(R, 1)
        return v

    # ------------------------------------------------------------------ minimum Bayes risk decoding
    def mbr_decode(self, img_input, a0, c0, start_seq, max_len, mbr, sample_step=0, constraints=None, consensus=None,
                   guidance=None, return_candidates=False):
        """Minimum Bayes risk decoding (``mbr``: a model_base.MBR, whose docstring defines it): per scan N = mbr.n_samples
        captions are sampled, and of them -- and the greedy caption, with mbr.include_greedy -- the one with the highest
        expected utility against the N samples is returned (definition: tnt_mbr_select_f32 in include/tnt_hip.h).
        Candidate c < N is exactly what sample_predict(..., temperature, top_k, top_p of ``mbr``, sample_step=sample_step
        + c) draws: the same captured decode replayed with another stream step; candidate N is greedy_predict's caption,
        a hypothesis only.  Each decode's ids are copied on the device into slot c of one (Nc, max_len, rows) buffer, and one
        tnt_mbr_select_f32 launch chooses: no token id visits the host before it.  ``constraints``, ``consensus``,
        ``guidance`` go to every candidate decode unchanged; with consensus or guidance the launch reads the M mixed rows of
        the G * M member rows.  Refused: max_len > 64 (ValueError), a data-parallel model (NotImplementedError).
        Returns (ids (M, max_len, 1) int64, info): info["expected"] (M, Nc) float32, info["best"] (M,) int32, and with
        ``return_candidates`` info["candidates"] (M, Nc, max_len) int64."""
        if not isinstance(mbr, MBR):
            raise ValueError(f"mbr must be a model_base.MBR, got {mbr!r}")
        if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or not 1 <= max_len <= mbr.MAX_LEN:
            raise ValueError(f"mbr_decode holds at most {mbr.MAX_LEN} tokens per caption: max_len must be an int in "
                             f"[1, {mbr.MAX_LEN}], got {max_len!r}")
        if isinstance(sample_step, bool) or not isinstance(sample_step, (int, np.integer)):
            raise ValueError(f"sample_step must be an int, got {sample_step!r}")
        if self.grad_sync is not None:
            raise NotImplementedError("mbr_decode has no data-parallel schedule: decode on one device")
        max_len, N, Nc = int(max_len), mbr.n_samples, mbr.n_candidates
        M = int(np.asarray(start_seq).reshape(-1).shape[0])
        kw = dict(constraints=constraints, consensus=consensus, guidance=guidance)
        st = None
        for c in range(Nc):
            filt = (mbr.temperature, mbr.top_k, mbr.top_p, int(sample_step) + c) if c < N else None
            ids = self._mbr_candidate(img_input, a0, c0, start_seq, max_len, filt, **kw)      # (max_len, rows) int32, static
            if st is None:
                st = self._mbr_state(M, Nc, max_len, int(ids.shape[1]))
            st["cand"][c].copy_(ids)
        rows = st["cand"].shape[2]
        self.be.mbr_select(st["cand"], rows, M, Nc, N, max_len, mbr.end_id, mbr.order, mbr.kind, st["expected"], st["best"],
                           st["out"], M)
        info = dict(expected=st["expected"].cpu().numpy(), best=st["best"].cpu().numpy())
        if return_candidates:
            info["candidates"] = st["cand"][:, :, :M].permute(2, 0, 1).contiguous().cpu().numpy().astype(np.int64)
        return st["out"].t().contiguous().cpu().numpy().astype(np.int64)[:, :, None], info

    def _mbr_candidate(self, img_input, a0, c0, start_seq, max_len, filt, constraints=None, consensus=None, guidance=None):
        """one candidate decode of mbr_decode: sample_predict's decode with ``filt`` = (temperature, top_k, top_p,
        sample_step), greedy_predict's with None.  Returns the decode's static device ids (max_len, rows) int32"""
        raise NotImplementedError(f"{type(self).__name__} has no minimum Bayes risk decoding")

    def _mbr_state(self, M, Nc, max_len, rows):
        """static buffers per (M, Nc, max_len, rows): cand (Nc, max_len, rows) int32, the candidates' ids; expected (M, Nc);
        best (M,) int32; out (max_len, M) int32, the chosen captions"""
        bufs = self._decode_bufs("_mbr_bufs")
        key = (M, Nc, max_len, rows)
        if key not in bufs:
            f, i32 = self._f, torch.int32
            bufs[key] = dict(cand=f(Nc, max_len, rows, dtype=i32), expected=f(M, Nc), best=f(M, dtype=i32),
                             out=f(max_len, M, dtype=i32))
        return bufs[key]

    def _dp_mean_logs(self, logs):
        """epoch logs averaged over the data-parallel ranks (same keys on every rank, sorted)"""
        import torch.distributed as dist
        keys = sorted(logs)
        vals = _dp_reduce([logs[k] for k in keys], dist.ReduceOp.SUM)
        return {k: v / self.dp_world for k, v in zip(keys, vals)}

    def _dp_any(self, flag):
        import torch.distributed as dist
        return _dp_reduce([1.0 if flag else 0.0], dist.ReduceOp.MAX)[0] > 0

    # ------------------------------------------------------------------ fit loop
    def fit(self, x=None, epochs=1, steps_per_epoch=None, batch_size=None, callbacks=None, validation_data=None,
            validation_steps=None, initial_epoch=0, verbose=1, keras_last_batch_logs=False, validation_averaged=False,
            class_weight=None, validation_captions=None, **kw):
        """model.fit(generator, epochs, steps_per_epoch, batch_size, callbacks, validation_data,
        validation_steps, initial_epoch) -- main.py:269-281.  Honours the keras callback protocol
        (on_train_begin, on_epoch_begin, on_train_batch_end, on_test_batch_end, on_epoch_end,
        on_train_end; Callbacks/EpochLoss.py:21-52).
        Epoch logs: the MEAN of the per-batch logs (what keras' compiled metrics report).  The reference's models
        override train_step / test_step and return plain tensors, for which Keras 2.4 hands ``on_epoch_end`` the
        LAST batch's values -- ``keras_last_batch_logs=True`` reproduces that (it matters to
        ModelCheckpoint(save_best_only) / EarlyStopping on ``val_loss``); the mean is the default because it is
        what those callbacks are meant to see.
        Data parallel: the epoch logs are averaged over the ranks and ``stop_training`` is OR-ed before the
        callbacks' decision takes effect, so every rank leaves the loop in the same epoch.
        ``validation_averaged=True`` (optimizers.MovingAverage / SWA): the validation pass of every epoch runs inside
        ``averaged_weights()``, so the ``val_*`` logs are the averaged model's.
        ``class_weight`` (keras: an ``{id: weight}`` dict; an array of V weights is accepted too): ``set_class_weight`` before
        the first step; None leaves the model's weights as they are.
        Gradient accumulation (optimizer gradient_accumulation_steps=k): ``steps_per_epoch`` counts micro-steps, an update
        is applied every k-th, and a window left open at the end of an epoch carries over into the next.
        ``validation_captions`` (evaluate.CaptionValidation, whose docstring defines it): behind the test_step pass of an
        epoch, and inside the same ``validation_averaged`` context, every validation batch is decoded and the captions are
        scored on the device; the epoch logs (``history``, and what the callbacks see) gain ``val_bleu4`` / ``val_rouge_l`` /
        ``val_cider_d``, each the mean of the per-caption scores.  One device only.  None: the launches and logs as they are."""
        if validation_captions is not None:
            from .evaluate import CaptionValidation
            if not isinstance(validation_captions, CaptionValidation):
                raise ValueError(f"validation_captions must be None or an evaluate.CaptionValidation, got "
                                 f"{validation_captions!r}")
            if self.dp_world > 1:
                raise NotImplementedError("fit(validation_captions=...) has no data-parallel schedule: validate on one device")
            if validation_data is None:
                raise ValueError("fit(validation_captions=...) needs validation_data")
            validation_captions.check_model(self)
        if class_weight is not None:
            self.set_class_weight(class_weight)
        if validation_averaged and self.average is None:
            raise ValueError("fit(validation_averaged=True) needs a model compiled with an averaging optimizer "
                             "(optimizers.MovingAverage / SWA)")
        callbacks = list(callbacks or [])
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            else:
                cb.model = self
        history = {}
        _call(callbacks, "on_train_begin", {})
        self.stop_training = False
        for epoch in range(initial_epoch, epochs):
            _call(callbacks, "on_epoch_begin", epoch, {})
            n = len(x) if steps_per_epoch is None else steps_per_epoch
            sums, last, t0 = {}, {}, time.time()
            for b in range(n):
                _call(callbacks, "on_train_batch_begin", b, {})
                try:
                    logs = self.train_step(x[b]).as_floats()
                except DeviceGuardError:        # the step left the model untouched and the fallback is in place: redo it
                    logs = self.train_step(x[b]).as_floats()
                for k, v in logs.items():
                    sums[k] = sums.get(k, 0.0) + v
                last = logs
                _call(callbacks, "on_train_batch_end", b, logs)
            elogs = dict(last) if keras_last_batch_logs else {k: v / max(n, 1) for k, v in sums.items()}
            if validation_data is not None:
                nv = len(validation_data) if validation_steps is None else validation_steps
                vs, vlast = {}, {}
                with (self.averaged_weights() if validation_averaged else nullcontext()):
                    for b in range(nv):
                        try:
                            logs = self.test_step(validation_data[b]).as_floats()
                        except DeviceGuardError:
                            logs = self.test_step(validation_data[b]).as_floats()
                        for k, v in logs.items():
                            vs[k] = vs.get(k, 0.0) + v
                        vlast = logs
                        _call(callbacks, "on_test_batch_end", b, logs)
                    vcap = validation_captions.epoch_logs(self, validation_data, nv) if validation_captions is not None else {}
                elogs.update({f"val_{k}": v for k, v in vlast.items()} if keras_last_batch_logs else
                             {f"val_{k}": v / max(nv, 1) for k, v in vs.items()})
                elogs.update(vcap)
            if self.dp_world > 1:
                elogs = self._dp_mean_logs(elogs)
            if verbose:
                print(f"epoch {epoch + 1}/{epochs} - {time.time() - t0:.1f}s - " +
                      " - ".join(f"{k}: {v:.4f}" for k, v in elogs.items()))
            for k, v in elogs.items():
                history.setdefault(k, []).append(v)
            self.check_device_errors()
            _call(callbacks, "on_epoch_end", epoch, elogs)
            if hasattr(x, "on_epoch_end"):
                x.on_epoch_end()
            if self.dp_world > 1:
                self.stop_training = self._dp_any(self.stop_training)
            if self.stop_training:
                break
        _call(callbacks, "on_train_end", {})
        return history


def _dp_reduce(values, op):
    import torch.distributed as dist
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor(values, dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=op)
    return t.cpu().tolist()


def _call(callbacks, name, *args):
    for cb in callbacks:
        fn = getattr(cb, name, None)
        if fn is not None:
            fn(*args)
