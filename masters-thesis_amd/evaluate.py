"""Decode / evaluation side of the reference, output-format compatible.

* ``eval_model`` / ``eval_fc_model``  -- AttemptFour/eval.py:148-216: run the generator through
  ``model.greedy_predict`` and write ``output_captions_<epoch>.npy``, ``output_captions_raw_<epoch>.npy``,
  ``attention_scores_<epoch>.npy`` and ``tokenizer.json`` with the reference's array layouts, so the
  thesis' analysis scripts keep working.
* ``beam_captions``                   -- the best beam-search caption of either model (``beam_search``), from the
  tokenizer's <start> / <end> indices.
* ``distinct_n``                      -- distinct n-grams / n-grams over a list of captions: the variety of an n-best list
  (diverse beam search, ``beam_search(diversity=model_base.BeamDiversity(...))``).
* ``ids_to_captions``                 -- tokenizer.sequences_to_texts with the <start>/<end>/<pad> handling of
  ThinkAndTell/evaluate.py:178-201.
* ``sentence_bleu`` / ``bleu_scores`` -- ThinkAndTell/img_evaluate.py:212-250 calls
  nltk.translate.bleu_score.sentence_bleu(references, candidate, weights, SmoothingFunction().method1);
  nltk is not installable here, so the published algorithm (Papineni et al. 2002; Chen & Cherry 2014 method 1:
  a zero n-gram match count becomes epsilon = 0.1) is restated.  PARITY UNPINNED against nltk itself; pinned by
  the worked example of the nltk documentation (tests/test_data_fit.py).
* ``RewardTable`` / ``device_scores``   -- CiderD's document frequencies as the sorted key / idf table that
  tnt_caption_reward_f32 reads (``SelfCritical(score_on="device")``), and that kernel's scores of lists of token ids.
* ``lcs_length`` / ``rouge_l``          -- ROUGE-L (Lin 2004) with the choices of the COCO caption suite's scorer
  (AttemptFour/metric_suit.py runs pycocoevalcap's Rouge): the F-score at beta = 1.2 of the best LCS precision and the
  best LCS recall over the references, each maximised on its own.  tnt_caption_rouge_f32 is the same definition on the
  device (``device_scores(kind="rouge-l")``, ``SelfCritical(reward="rouge-l")``).
* ``CaptionValidation``                 -- caption metrics of the decoded validation set in ``fit``'s epoch logs
  (``fit(validation_captions=...)``): val_bleu4, val_rouge_l, val_cider_d, scored on the device.
* ``SemanticBank`` / ``semantic_retrieve`` / ``semantic_identification`` -- nearest-neighbour retrieval and identification in
  sentence-embedding space for nic.NIC(semantic=...): Model/guse.py's "KNN is used to find a known GUSE vector", which the
  reference never finishes; the similarities and the selection run on the device (tnt_cosine_topk_f32).
Host-side Python throughout: nothing here is on the per-step hot path (``pack_references`` fills a pinned array per
device-scored self-critical step).
"""
import math
import os
from collections import Counter

import numpy as np


def _con_kw(constraints, consensus=None, guidance=None):
    """the ``constraints=`` / ``consensus=`` / ``guidance=`` keywords of a decode call, each passed only when set: a model
    without constrained, consensus or guided decoding then refuses the call instead of ignoring the keyword"""
    kw = {} if constraints is None else {"constraints": constraints}
    if consensus is not None:
        kw["consensus"] = consensus
    if guidance is not None:
        kw["guidance"] = guidance
    return kw


def _n_start(features, consensus):
    """entries of start_seq for a batch of scans: one per scan, or with consensus one per image (the batch holds
    members * M rows, member-major; a batch that does not divide is left to the decode to refuse)"""
    n = int(features.shape[0])
    return n if consensus is None else max(n // int(consensus.members), 1)


def eval_model(model, data_generator, tokenizer, config, out_path, epoch, add_name="", constraints=None, consensus=None,
               guidance=None):
    """eval.py:148-194.  greedy_predict returns (words (B,T,1), probs (B,T,V), alpha (T,B,R,1), s); the files hold
    outputs (n,T,1), outputs_raw (n,T,V) and attention_scores (n,T,R,1) (eval.py:172-174).  ``constraints``
    (model_base.DecodeConstraints) goes to greedy_predict: outputs_raw then holds the constrained distributions.
    ``consensus`` (model_base.Consensus) goes to greedy_predict too: every batch then holds members * M scans, member-major,
    outputs and outputs_raw are per image (the mixtures) and attention_scores stay per member row.
    ``guidance`` (model_base.Guidance) goes to greedy_predict as well: outputs_raw then holds the guided distributions, and
    attention_scores keep the scans' rows (the null scans' rows behind them are dropped)."""
    outs, raws, attns = [], [], []
    for i in range(len(data_generator)):
        sample = data_generator[i]
        features, _, a0, c0 = sample[0][:4]
        start_seq = np.repeat([tokenizer.word_index["<start>"]], _n_start(features, consensus))
        words, probs, alpha, _ = model.greedy_predict(features, a0, c0, start_seq, config["max_length"], config["units"],
                                                      tokenizer, return_s=False,     # eval.py never reads `s`
                                                      **_con_kw(constraints, consensus, guidance))
        if guidance is not None:
            alpha = alpha[:, :words.shape[0]]
        outs.append(words); raws.append(probs); attns.append(alpha)
    outputs = np.concatenate(outs, axis=0)
    outputs_raw = np.concatenate(raws, axis=0)
    attention_scores = np.swapaxes(np.concatenate(attns, axis=1), 0, 1)
    os.makedirs(out_path, exist_ok=True)
    np.save(os.path.join(out_path, f"output_captions_{epoch}{add_name}.npy"), outputs)
    np.save(os.path.join(out_path, f"output_captions_raw_{epoch}{add_name}.npy"), outputs_raw)
    np.save(os.path.join(out_path, f"attention_scores_{epoch}{add_name}.npy"), attention_scores)
    with open(os.path.join(out_path, "tokenizer.json"), "w") as f:
        f.write(tokenizer.to_json())
    return outputs, attention_scores


def eval_fc_model(model, data_generator, tokenizer, config, out_path, epoch, add_name="", constraints=None,
                  consensus=None, guidance=None):
    """eval.py:196-216: greedy_predict_fc returns ids (T,B,1); the file holds (n,T,1).  ``constraints``, ``consensus`` and
    ``guidance`` go to the model's greedy_predict (a model whose decode has no such keyword, NICfc among them, refuses the call)."""
    outs = []
    for i in range(len(data_generator)):
        sample = data_generator[i]
        features, _, a0, c0 = sample[0][:4]
        start_seq = np.repeat([tokenizer.word_index["<start>"]], _n_start(features, consensus))
        outs.append(model.greedy_predict(features, a0, c0, start_seq, config["max_length"], config["units"], tokenizer,
                                         **_con_kw(constraints, consensus, guidance)))
    all_outputs = np.swapaxes(np.concatenate(outs, axis=1), 0, 1)
    os.makedirs(out_path, exist_ok=True)
    np.save(os.path.join(out_path, f"output_captions_{epoch}{add_name}.npy"), all_outputs)
    with open(os.path.join(out_path, "tokenizer.json"), "w") as f:
        f.write(tokenizer.to_json())
    return all_outputs


def ids_to_captions(ids, tokenizer, end_token="<end>", drop=("<start>", "<pad>")):
    """(n,T[,1]) ids -> list of token lists, cut at the first <end> (ThinkAndTell/evaluate.py:178-201); id 0 is
    padding."""
    ids = np.asarray(ids)
    if ids.ndim == 3:
        ids = ids[:, :, 0]
    caps = []
    for row in ids:
        words = []
        for i in row:
            w = tokenizer.index_word.get(int(i)) if int(i) != 0 else None
            if w is None or w in drop:
                continue
            if w == end_token:
                break
            words.append(w)
        caps.append(words)
    return caps


def beam_captions(model, features, a0, c0, tokenizer, max_len, beam_width=5, length_penalty=0.0, end_token="<end>",
                  constraints=None, consensus=None, diversity=None, guidance=None):
    """Beam-search captions of either model (nic.NIC or lc_nic.NIC ``beam_search``): every caption starts at the
    tokenizer's "<start>" index and a beam ends at ``end_token``'s index.  Returns (ids (B, max_len) int64 of each
    sample's best beam, captions: token lists cut at ``end_token`` as ids_to_captions cuts).  ``constraints``
    (model_base.DecodeConstraints) goes to beam_search; its min_length counts against ``end_token``'s index.
    ``consensus`` (model_base.Consensus) goes to beam_search too: ``features`` then holds members * M scans, member-major,
    and one caption per image comes back.  ``diversity`` (model_base.BeamDiversity) goes to beam_search as well; the
    caption returned is group 0's best, the plain search of width beam_width / groups (call beam_search for all of them).
    ``guidance`` (model_base.Guidance) goes to beam_search too: the beams are scored by the guided distributions."""
    end_id = int(tokenizer.word_index[end_token])
    start = np.full(_n_start(features, consensus), int(tokenizer.word_index["<start>"]), np.int64)
    seqs, _ = model.beam_search(features, a0, c0, start, max_len, beam_width=beam_width, end_id=end_id,
                                length_penalty=length_penalty, **_con_kw(constraints, consensus, guidance),
                                **({} if diversity is None else {"diversity": diversity}))
    ids = np.ascontiguousarray(seqs[:, 0, :]).astype(np.int64)
    return ids, ids_to_captions(ids, tokenizer, end_token=end_token)


def mbr_captions(model, features, a0, c0, tokenizer, max_len, mbr, sample_step=0, end_token="<end>", constraints=None,
                 consensus=None, guidance=None):
    """Minimum Bayes risk captions of either model (nic.NIC or lc_nic.NIC ``mbr_decode``; ``mbr``: a model_base.MBR, whose
    end_id must be ``end_token``'s index): every caption starts at the tokenizer's "<start>" index.  Returns (ids (B,
    max_len) int64 of each scan's chosen candidate, captions: token lists cut at ``end_token`` as ids_to_captions cuts,
    info: mbr_decode's, the expected utilities (B, Nc) and the chosen index (B,)).  ``constraints``, ``consensus`` and
    ``guidance`` go to mbr_decode, and through it to every candidate decode; with consensus ``features`` holds members * M
    scans, member-major, and one caption per image comes back."""
    end_id = int(tokenizer.word_index[end_token])
    if int(mbr.end_id) != end_id:
        raise ValueError(f"mbr.end_id = {mbr.end_id} is not the index of {end_token!r} ({end_id})")
    start = np.full(_n_start(features, consensus), int(tokenizer.word_index["<start>"]), np.int64)
    words, info = model.mbr_decode(features, a0, c0, start, max_len, mbr, sample_step=sample_step,
                                   **_con_kw(constraints, consensus, guidance))
    ids = np.ascontiguousarray(words[:, :, 0]).astype(np.int64)
    return ids, ids_to_captions(ids, tokenizer, end_token=end_token), info


def distinct_n(captions, n):
    """distinct-n (Li et al. 2016) of a list of token sequences (lists of words or ids): the number of distinct n-grams
    over all the sequences divided by the total number of n-grams; 0.0 when no sequence holds an n-gram.  1.0: no n-gram
    occurs twice; near 1 / len(captions): the sequences are copies of each other."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"n must be an int >= 1, got {n!r}")
    grams = [tuple(cap[i:i + n]) for cap in (list(c) for c in captions) for i in range(len(cap) - n + 1)]
    return len(set(grams)) / len(grams) if grams else 0.0


def repeat_rate(captions):
    """The share of tokens that repeat an earlier token of the same caption, over a list of token sequences (lists of
    words or ids, cut at the end token as ``ids_to_captions`` cuts, like those ``distinct_n`` takes): sum over the
    captions of (length - number of distinct tokens), divided by the total number of tokens; 0.0 when there is no
    token.  This is the quantity ``CategoricalCrossentropy(unlikelihood=...)`` acts on: every repeated token was a
    negative candidate at its position.  Host only."""
    caps = [list(c) for c in captions]
    total = sum(len(c) for c in caps)
    return sum(len(c) - len(set(c)) for c in caps) / total if total else 0.0


def simple_eval(model, betas, target, tokenizer=None, temperature=1.0, sample_step=0, end_token="<end>", top_k=0,
                top_p=1.0, constraints=None):
    """ThinkAndTell/evaluate.py:261-284 (`simple_eval`): one teacher-forced forward of the caption generator, then one
    categorical draw per position from the logits (tf.random.categorical(logits, 1)); the caption is cut at the first
    <end>.  The draw runs on the device (tnt_sample_rows_f32, Philox stream (seed, S_SAMPLE, sample_step)).
    ``top_k`` / ``top_p`` filter the draw (tnt_sample_topkp_f32 on the same stream; the defaults 0 / 1 are off).
    ``constraints`` (model_base.DecodeConstraints; None or neutral: the draw above): the positions are drawn one after the
    other instead, position t from its teacher-forced logits constrained by the tokens drawn at positions 0 .. t-1
    (tnt_decode_constrain_f32 in front of each draw; the history is the draws, not the target), on the stream
    (seed, S_SAMPLE + t, sample_step), element b; more than 32 positions are refused (ValueError), the streams behind
    S_SAMPLE + 31 belong to other sites.  ``end_token``'s index serves min_length when the object names none.
    Returns (ids (B, T+1) int64, captions or None)."""
    import torch
    from . import ops
    from .model_base import S_SAMPLE, SS_MAX_POSITIONS, check_sampling
    top_k, top_p, _ = check_sampling(top_k, top_p, temperature)
    logits = model((betas, None, target), training=False)                 # (B, T+1, V), device tensor
    Bn, Tn, V = logits.shape
    end_id = int(tokenizer.word_index.get(end_token, -1)) if tokenizer is not None else -1
    con = model._constrain(constraints, Bn, Tn, 1, end_id) if constraints is not None else None
    if con is not None and Tn > SS_MAX_POSITIONS:
        raise ValueError(f"simple_eval with constraints draws at most {SS_MAX_POSITIONS} positions (one Philox site each), "
                         f"got {Tn}")
    flat = logits.reshape(Bn * Tn, V).contiguous()
    ids = torch.zeros(Bn * Tn, dtype=torch.int32, device=flat.device)
    if con is not None:
        rows = logits.permute(1, 0, 2).contiguous()                      # (T+1, B, V): one position's rows side by side
        ids = ids.view(Tn, Bn)
        for t in range(Tn):
            con.step(t, rows[t], V, ids[t - 1] if t > 0 else None)
            ops.backend().sample_topkp(rows[t], ids[t], Bn, V, V, temperature, top_k, top_p, True, model.seed, S_SAMPLE + t,
                                       sample_step)
        ids = ids.t().contiguous().view(-1)
    elif top_k == 0 and top_p == 1.0:
        ops.backend().sample_rows(flat, ids, Bn * Tn, V, V, temperature, True, model.seed, S_SAMPLE, sample_step)
    else:
        ops.backend().sample_topkp(flat, ids, Bn * Tn, V, V, temperature, top_k, top_p, True, model.seed, S_SAMPLE,
                                   sample_step)
    ids = ids.view(Bn, Tn).cpu().numpy().astype(np.int64)
    caps = None
    if tokenizer is not None:
        caps = []
        for row in ids:
            words = []
            for i in row:
                w = tokenizer.index_word.get(int(i), "<unk>")
                words.append(w)
                if w == end_token:
                    break
            caps.append(words)
    return ids, caps


def _ngrams(seq, n):
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


def sentence_bleu(references, hypothesis, weights=(0.25, 0.25, 0.25, 0.25), smoothing="method1", epsilon=0.1):
    """BLEU of one tokenised hypothesis against tokenised references: clipped n-gram precisions, geometric mean
    with ``weights``, brevity penalty against the closest reference length.  smoothing=None: any zero precision
    gives 0; "method1": zero match counts are replaced by ``epsilon`` (Chen & Cherry 2014)."""
    hyp_len = len(hypothesis)
    if hyp_len == 0:
        return 0.0
    p = []
    for n in range(1, len(weights) + 1):
        hyp = _ngrams(hypothesis, n)
        max_ref = Counter()
        for ref in references:
            for g, c in _ngrams(ref, n).items():
                max_ref[g] = max(max_ref[g], c)
        num = sum(min(c, max_ref[g]) for g, c in hyp.items())
        den = max(1, sum(hyp.values()))
        p.append((num, den))
    if p[0][0] == 0:                       # no unigram overlap at all
        return 0.0
    ref_len = min((len(r) for r in references), key=lambda rl: (abs(rl - hyp_len), rl))
    bp = 1.0 if hyp_len > ref_len else math.exp(1.0 - ref_len / hyp_len)
    s = 0.0
    for w, (num, den) in zip(weights, p):
        if num == 0:
            if smoothing is None:
                return 0.0
            num = epsilon
        s += w * math.log(num / den)
    return bp * math.exp(s)


def bleu_scores(references, candidate):
    """The four scores of ThinkAndTell/img_evaluate.py:245-248 (BLEU-1..4, cumulative weights, method 1)."""
    ws = [(1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0), (0.25, 0.25, 0.25, 0.25)]
    return tuple(sentence_bleu(references, candidate, weights=w) for w in ws)


class CiderD:
    """CIDEr-D (Vedantam et al. 2015) of tokenised captions, restated from the published definition with the choices of
    coco-caption's CiderD scorer: n-grams of n = 1..4, each with its own tf-idf vector (tf = the raw n-gram count,
    idf = log(number of documents) - log(max(1, df)), df = the number of documents whose references contain the n-gram;
    a document is one scan's set of references); the numerator is clipped, each n-gram of the candidate contributing
    min(candidate, reference) x reference tf-idf, over the product of the two vector norms; a Gaussian length penalty
    exp(-(l_c - l_r)^2 / (2 sigma^2)), sigma = 6; the scores are averaged over n and over the references and multiplied by 10.
    ``corpus`` (a list of documents, each a list of tokenised references): the document frequencies, fixed for this
    scorer, and each reference's vectors are cached across calls.  ``corpus=None``: the frequencies come from the
    documents of each ``batch_scores`` call, coco-caption's behaviour (with one document every idf is 0 and so is every
    score).  PARITY UNPINNED against pycocoevalcap itself, which is not available here; pinned by hand-computed cases
    (tests/test_host_scst.py).  Host-side Python."""

    def __init__(self, corpus=None, n=4, sigma=6.0):
        self.n, self.sigma = int(n), float(sigma)
        self._cache = {}
        self._df = self._log_docs = None
        if corpus is not None:
            self._df, self._log_docs = self._doc_freq(corpus)

    def _counts(self, seq):
        seq = tuple(int(w) if isinstance(w, (int, np.integer)) else w for w in seq)
        return [_ngrams(seq, k) for k in range(1, self.n + 1)], len(seq)

    def _doc_freq(self, docs):
        df = Counter()
        ndoc = 0
        for refs in docs:
            ndoc += 1
            seen = set()
            for ref in refs:
                for c in self._counts(ref)[0]:
                    seen.update(c)
            df.update(seen)
        return df, math.log(float(max(ndoc, 1)))

    def _vec(self, seq, df, log_docs):
        """(per-n tf-idf dicts, per-n squared norms, length)"""
        counts, length = self._counts(seq)
        vecs, sq = [], []
        for c in counts:
            v = {g: float(tf) * (log_docs - math.log(max(1.0, float(df.get(g, 0))))) for g, tf in c.items()}
            vecs.append(v)
            sq.append(sum(x * x for x in v.values()))
        return vecs, sq, length

    def _sim(self, hyp, ref):
        (vh, sh, lh), (vr, sr, lr) = hyp, ref
        pen = math.exp(-((lh - lr) ** 2) / (2.0 * self.sigma ** 2))
        total = 0.0
        for k in range(self.n):
            num = sum(min(x, vr[k].get(g, 0.0)) * vr[k].get(g, 0.0) for g, x in vh[k].items())
            den = sh[k] * sr[k]
            total += (num / math.sqrt(den) if den != 0.0 else 0.0) * pen
        return total / self.n

    def _score(self, hyp, refs):
        if not refs:
            return 0.0
        return 10.0 * sum(self._sim(hyp, r) for r in refs) / len(refs)

    def batch_scores(self, candidates, references):
        """candidates: one list of candidate token sequences per document; references: one list of reference token
        sequences per document.  Returns one float64 array of scores per document."""
        if len(candidates) != len(references):
            raise ValueError(f"{len(candidates)} candidate lists for {len(references)} documents")
        if self._df is None:
            df, log_docs = self._doc_freq(references)
            ref_vec = lambda r: self._vec(r, df, log_docs)
        else:
            df, log_docs = self._df, self._log_docs

            def ref_vec(r):
                key = tuple(r)
                v = self._cache.get(key)
                if v is None:
                    v = self._cache[key] = self._vec(r, df, log_docs)
                return v
        out = []
        for cands, refs in zip(candidates, references):
            rv = [ref_vec(r) for r in refs]
            out.append(np.array([self._score(self._vec(c, df, log_docs), rv) for c in cands], np.float64))
        return out

    def __call__(self, candidate, references):
        """the score of one candidate against its references (one document: the scorer's corpus frequencies, or,
        without a corpus, these references alone)"""
        return float(self.batch_scores([[candidate]], [references])[0][0])


def lcs_length(a, b):
    """the length of the longest common subsequence of two token sequences (words or ids), the O(len(a) * len(b)) table
    kept one row at a time"""
    a, b = list(a), list(b)
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            diag, row[j + 1] = row[j + 1], (diag + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


ROUGE_BETA = 1.2        # pycocoevalcap's Rouge().beta


def rouge_l(references, hypothesis, beta=ROUGE_BETA):
    """ROUGE-L of one tokenised hypothesis against tokenised references, pycocoevalcap's Rouge.calc_score: over the
    references that hold a word, P = max lcs / len(hypothesis) and R = max lcs / len(reference), each maximum on its own (they
    may come from different references), and ((1 + beta^2) P R) / (R + beta^2 P); 0.0 for an empty hypothesis, no such
    reference or no common word.  The operation order is tnt_caption_rouge_f32's (include/tnt_hip.h).  PARITY UNPINNED
    against pycocoevalcap itself, which is not available here; pinned by hand-computed cases (tests/test_host_rouge.py)."""
    beta = float(beta)
    if not (beta > 0.0 and math.isfinite(beta * beta)):
        raise ValueError(f"beta must be a finite float > 0, got {beta!r}")
    hyp = list(hypothesis)
    if not hyp:
        return 0.0
    P = R = 0.0
    for ref in references:
        ref = list(ref)
        if not ref:
            continue
        n = lcs_length(hyp, ref)
        P, R = max(P, n / len(hyp)), max(R, n / len(ref))
    if P == 0.0:
        return 0.0
    b2 = beta * beta
    return (((1.0 + b2) * P) * R) / (R + b2 * P)


# ---------------------------------------------------------------------------------------------------- rewards on the device
REWARD_KINDS = {"cider-d": 0, "bleu4": 1}                              # tnt_caption_reward_f32's kind
ROUGE_KIND = "rouge-l"                                                 # tnt_caption_rouge_f32: an entry of its own
DEVICE_KINDS = tuple(REWARD_KINDS) + (ROUGE_KIND,)
REWARD_MAX_SAMPLES, REWARD_MAX_REFS, REWARD_MAX_LEN = 16, 8, 64        # tnt_caption_reward_f32's limits: K, M, T and Lr


def gram_key(gram):
    """the 64-bit table key of a k-gram (k <= 4) of token ids in [1, 65535]: w0 | w1<<16 | w2<<32 | w3<<48, missing high
    words zero.  Id 0 never occurs inside a gram, so the orders share one key space."""
    key = 0
    for i, w in enumerate(gram):
        key |= int(w) << (16 * i)
    return key


class RewardTable:
    """The document frequencies of ``CiderD(corpus)`` as tnt_caption_reward_f32 reads them (definition: include/tnt_hip.h):
    ``keys`` uint64, strictly ascending (gram_key of every n-gram of the corpus, n = 1..4), ``idf`` float64 with
    idf = log(ndoc) - log(max(1, df)) computed exactly as CiderD._vec does, ``params`` = {log(ndoc), sigma} float64.
    A gram that is not in the table has df = 0: its idf is log(ndoc).  Token ids outside [1, 65535] (a vocabulary above
    65536; ``vocab_size`` states it without a corpus that uses it) are refused: a key holds 16 bits per word.
    ``device(dev)`` uploads the three arrays once and caches them."""

    def __init__(self, corpus, n=4, sigma=6.0, vocab_size=None):
        if int(n) != 4:
            raise ValueError(f"the device scorer's n-gram order is 4, got n = {n!r}")
        if vocab_size is not None and int(vocab_size) > 65536:
            raise ValueError(f"a reward table packs 16 bits per token id: vocab_size {vocab_size} is above 65536")
        cd = CiderD(corpus, n=4, sigma=sigma)
        if cd._df is None:
            raise ValueError("a reward table needs a corpus (a list of documents, each a list of tokenised references)")
        entries = []
        for gram, df in cd._df.items():
            for w in gram:
                if not isinstance(w, (int, np.integer)) or not 1 <= w <= 65535:
                    raise ValueError(f"a reward table packs 16 bits per token id, each in [1, 65535]: the corpus holds {w!r}")
            entries.append((gram_key(gram), cd._log_docs - math.log(max(1.0, float(df)))))
        entries.sort()
        self.keys = np.array([k for k, _ in entries], np.uint64)
        self.idf = np.array([v for _, v in entries], np.float64)
        self.params = np.array([cd._log_docs, cd.sigma], np.float64)
        self._dev = {}

    def __len__(self):
        return int(self.keys.size)

    def device(self, dev):
        """(keys, idf, params) on ``dev``, uploaded once; keys travel as the int64 tensor with the same bits"""
        import torch
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = (torch.from_numpy(self.keys.view(np.int64).copy()).to(dev),
                                  torch.from_numpy(self.idf.copy()).to(dev), torch.from_numpy(self.params.copy()).to(dev))
        return t


def pack_references(references, refs_out, n_out):
    """B lists of tokenised references into the zero-padded refs_out (B, M, Lr) int32 and n_out (B,) int32 (numpy arrays
    or CPU tensors' numpy views), tnt_caption_reward_f32's layout.  More than M references or a reference longer than Lr
    raises ValueError, before anything is written."""
    B, M, Lr = refs_out.shape
    if len(references) != B:
        raise ValueError(f"{len(references)} reference lists for {B} scans")
    docs = [[[int(w) for w in r] for r in doc] for doc in references]
    for doc in docs:
        if len(doc) > M:
            raise ValueError(f"the device scorer holds at most {M} references per scan, got {len(doc)}")
        for r in doc:
            if len(r) > Lr:
                raise ValueError(f"the device scorer holds at most {Lr} tokens per reference, got {len(r)}")
    refs_out[...] = 0
    for b, doc in enumerate(docs):
        n_out[b] = len(doc)
        for j, r in enumerate(doc):
            refs_out[b, j, :len(r)] = r


def device_scores(candidates, references, kind="cider-d", table=None, end_id=-1, device="cuda", beta=ROUGE_BETA):
    """The scores tnt_caption_reward_f32 gives lists of token ids: ``candidates`` one list of at most 16 candidate
    token sequences per document, ``references`` one list of at most 8 reference sequences per document, as
    CiderD.batch_scores takes them; sequences hold at most 64 tokens and are cut at their first ``end_id`` or 0
    (end_id < 0: only 0).  kind "cider-d" needs ``table`` (a RewardTable); "bleu4" takes none.  kind "rouge-l": the
    scores of tnt_caption_rouge_f32 at ``beta`` on the same buffers (``rouge_l``'s definition).  One launch with
    K = the largest candidate count; returns one float64 array of scores per document."""
    import torch
    from . import ops
    if kind not in DEVICE_KINDS:
        raise ValueError(f"kind must be one of {DEVICE_KINDS}, got {kind!r}")
    if kind == "cider-d" and not isinstance(table, RewardTable):
        raise ValueError("kind 'cider-d' needs table=RewardTable(corpus)")
    if len(candidates) != len(references):
        raise ValueError(f"{len(candidates)} candidate lists for {len(references)} documents")
    B = len(candidates)
    if B == 0:
        return []
    cands = [[[int(w) for w in c] for c in doc] for doc in candidates]
    K = max(1, max(len(doc) for doc in cands))
    T = max(1, max((len(c) for doc in cands for c in doc), default=1))
    if K > REWARD_MAX_SAMPLES or T > REWARD_MAX_LEN:
        raise ValueError(f"the device scorer holds at most {REWARD_MAX_SAMPLES} candidates per document of at most "
                         f"{REWARD_MAX_LEN} tokens, got {K} of {T}")
    M = max(1, max(len(doc) for doc in references))
    Lr = max(1, max((len(r) for doc in references for r in doc), default=1))
    if M > REWARD_MAX_REFS or Lr > REWARD_MAX_LEN:
        raise ValueError(f"the device scorer holds at most {REWARD_MAX_REFS} references per document of at most "
                         f"{REWARD_MAX_LEN} tokens, got {M} of {Lr}")
    refs, n_refs = np.zeros((B, M, Lr), np.int32), np.zeros(B, np.int32)
    pack_references(references, refs, n_refs)
    w = np.zeros((B * K, T + 1), np.int32)                 # column 0: the start token's place, never read
    for b, doc in enumerate(cands):
        for k, c in enumerate(doc):
            w[b * K + k, 1:1 + len(c)] = c
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fed, last = up(w[:, :T]), up(w[:, T])
    greedy = torch.zeros(T, B, dtype=torch.int32, device=dev)
    adv = torch.zeros(B * K, dtype=torch.float32, device=dev)
    score = torch.zeros(B, K + 1, dtype=torch.float64, device=dev)
    counted = torch.zeros(B * K, dtype=torch.int32, device=dev)
    keys, idf, params = table.device(dev) if kind == "cider-d" else (None, None, None)
    n_keys = len(table) if kind == "cider-d" else 0
    if n_keys == 0:
        keys = idf = None
    if kind == ROUGE_KIND:
        ops.backend().caption_rouge(fed, T, last, greedy, B, up(refs), up(n_refs), M, Lr, B, K, int(end_id), float(beta), 0,
                                    adv, score, counted)
    else:
        ops.backend().caption_reward(fed, T, last, greedy, B, up(refs), up(n_refs), M, Lr, keys, idf, n_keys, params, B, K,
                                     int(end_id), REWARD_KINDS[kind], 0, adv, score, counted)
    s = score.cpu().numpy()
    return [s[b, :len(doc)].copy() for b, doc in enumerate(cands)]


# ---------------------------------------------------------------------------------------------------- caption metrics in fit
class CaptionValidation:
    """Caption metrics of the decoded validation set in ``fit``'s epoch logs (``fit(validation_captions=...)`` of nic.NIC and
    lc_nic.NIC): what ModelCheckpoint(save_best_only=True, mode="max") and EarlyStopping(mode="max") select on in place of
    the teacher-forced ``val_loss``, which a decoder that learns the language prior and ignores the scan keeps lowering.
    After an epoch's test_step pass every validation batch is decoded in inference mode with the model's device decode,
    from column 0 of the batch's caption for its remaining positions; the ids stay on the device and are scored there as
    the "greedy" candidate of a reward launch whose one sample row is empty (tnt_caption_reward_f32 / tnt_caption_rouge_f32,
    score[:, 1]); one float64 sum per metric and batch is kept on the device and read at the end of the pass.  The decode
    takes its start tokens from the host: a batch of numpy arrays adds no synchronise, a batch of device tensors one small
    read per batch.
      end_id       the tokenizer's <end> index; a caption or a reference ends at its first end_id or 0
      metrics      of "bleu4" (log ``val_bleu4``), "rouge-l" (``val_rouge_l``), "cider-d" (``val_cider_d``; needs ``table``,
                   and is added when a table is given)
      table        a RewardTable: CIDEr-D's document frequencies
      references   one list of reference lists per validation batch (at most 8 per scan of at most 64 tokens); None: each
                   row's own caption, columns 1..
      decode       "greedy", or "beam" with ``beam_width`` (the best beam of beam_search, whose paths are back-tracked on the
                   host and sent back)
      constraints, guidance   model_base.DecodeConstraints / Guidance, handed to the decode
    Each value is the MEAN OF THE PER-CAPTION SCORES over the validation set (evaluate.sentence_bleu, rouge_l, CiderD per
    caption); val_bleu4 is therefore not corpus-level BLEU, which pools the n-gram counts of all captions first."""

    METRICS = ("bleu4", "rouge-l", "cider-d")
    DECODES = ("greedy", "beam")

    def __init__(self, end_id, metrics=("bleu4", "rouge-l"), table=None, references=None, decode="greedy", beam_width=None,
                 constraints=None, guidance=None):
        if isinstance(end_id, bool) or not isinstance(end_id, (int, np.integer)) or end_id < 1:
            raise ValueError(f"CaptionValidation end_id must be an int >= 1 (the <end> index), got {end_id!r}")
        metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
        for m in metrics:
            if m not in self.METRICS:
                raise ValueError(f"CaptionValidation metrics are of {self.METRICS}, got {m!r}")
        if table is not None and not isinstance(table, RewardTable):
            raise ValueError(f"table must be None or an evaluate.RewardTable, got {type(table).__name__}")
        if table is not None and "cider-d" not in metrics:
            metrics += ("cider-d",)
        if "cider-d" in metrics and table is None:
            raise ValueError("metric 'cider-d' needs table=RewardTable(corpus)")
        if not metrics:
            raise ValueError("CaptionValidation needs at least one metric")
        if decode not in self.DECODES:
            raise ValueError(f"decode must be one of {self.DECODES}, got {decode!r}")
        if decode == "beam":
            if isinstance(beam_width, bool) or not isinstance(beam_width, (int, np.integer)) or beam_width < 1:
                raise ValueError(f"decode='beam' needs beam_width, an int >= 1, got {beam_width!r}")
        elif beam_width is not None:
            raise ValueError("beam_width goes with decode='beam'")
        self.end_id, self.metrics, self.table, self.decode = int(end_id), metrics, table, decode
        self.beam_width = None if beam_width is None else int(beam_width)
        self.references = None if references is None else [[[[int(w) for w in r] for r in doc] for doc in batch]
                                                           for batch in references]
        self.constraints, self.guidance = constraints, guidance
        self._bufs, self._refs = {}, {}

    @staticmethod
    def log_name(metric):
        return "val_" + metric.replace("-", "_")

    def _decode_ids(self, model, x, a0, c0, start, max_len):
        """the decoded ids (max_len, ld >= B) int32 on the model's device, column b = scan b"""
        import torch
        kw = _con_kw(self.constraints, None, self.guidance)
        if self.decode == "greedy":
            return model._mbr_candidate(x, a0, c0, start, max_len, None, **kw)
        seqs, _ = model.beam_search(x, a0, c0, start, max_len, beam_width=self.beam_width, end_id=self.end_id, **kw)
        best = np.ascontiguousarray(np.asarray(seqs)[:, 0, :].T.astype(np.int32))
        return torch.from_numpy(best).to(model.device)

    def _batch_refs(self, model, index, cap, B):
        """(refs (B, M, Lr) int32, n_refs (B,)) on the device: the batch's reference lists, packed and uploaded once, or the
        rows' own captions"""
        import torch
        dev = model.device
        if self.references is None:
            own = cap[:, 1:].contiguous()
            return own.view(B, 1, own.shape[1]), torch.ones(B, dtype=torch.int32, device=dev)
        if index not in self._refs:
            docs = self.references[index]
            if len(docs) != B:
                raise ValueError(f"validation batch {index}: {len(docs)} reference lists for {B} scans")
            M = max(1, max(len(d) for d in docs))
            Lr = max(1, max((len(r) for d in docs for r in d), default=1))
            if M > REWARD_MAX_REFS or Lr > REWARD_MAX_LEN:
                raise ValueError(f"the device scorer holds at most {REWARD_MAX_REFS} references per scan of at most "
                                 f"{REWARD_MAX_LEN} tokens, got {M} of {Lr}")
            refs, n = np.zeros((B, M, Lr), np.int32), np.zeros(B, np.int32)
            pack_references(docs, refs, n)
            self._refs[index] = (torch.from_numpy(refs).to(dev), torch.from_numpy(n).to(dev))
        return self._refs[index]

    @staticmethod
    def check_model(model):
        """refuse, before any training, a model whose decode does not leave its ids on the device (fit calls this)"""
        from . import lc_nic, nic
        cls = type(model)
        # the device decode is nic.NIC's and lc_nic.NIC's; a subclass with a greedy decode of its own (fc_nic.NICfc) has none
        if not any(isinstance(model, base) and cls.greedy_predict is base.greedy_predict for base in (nic.NIC, lc_nic.NIC)):
            raise NotImplementedError(f"fit(validation_captions=...) decodes with the device decode of nic.NIC and lc_nic.NIC: "
                                      f"{type(model).__name__} has none")

    def epoch_logs(self, model, validation_data, steps):
        """decode and score ``steps`` validation batches; returns {log name: mean per-caption score}"""
        import torch
        from . import ops
        if self.references is not None and len(self.references) < steps:
            raise ValueError(f"references holds {len(self.references)} batches for {steps} validation batches")
        be, dev = ops.backend(), model.device
        sums, count = {m: [] for m in self.metrics}, 0
        for index in range(steps):
            x, cap, a0, c0 = validation_data[index][0][:4]
            # the start tokens go to the decode from the host: a batch that arrives as numpy keeps them there, a batch of
            # device tensors costs one small read (and so one synchronise) here
            start = cap[:, 0].cpu().numpy() if isinstance(cap, torch.Tensor) else np.asarray(cap)[:, 0]
            cap = model._to_dev(cap, torch.int32)
            B, L = int(cap.shape[0]), int(cap.shape[1]) - 1
            if not 1 <= L <= REWARD_MAX_LEN:
                raise ValueError(f"validation captions of {L + 1} columns: the device scorer holds 1 to {REWARD_MAX_LEN} decoded "
                                 f"positions behind the start token")
            ids = self._decode_ids(model, x, a0, c0, start, L)
            refs, n_refs = self._batch_refs(model, index, cap, B)
            st = self._bufs.get((B, L))
            if st is None:
                z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)
                # the launch's one sample row per scan stays empty (all zeros): its score is 0 and is not read
                st = self._bufs[(B, L)] = dict(fed=z(B, L), last=z(B), counted=z(B), adv=z(B, dtype=torch.float32),
                                               score=z(B, 2, dtype=torch.float64))
            M, Lr = int(refs.shape[1]), int(refs.shape[2])
            for m in self.metrics:
                if m == ROUGE_KIND:
                    be.caption_rouge(st["fed"], L, st["last"], ids, int(ids.shape[1]), refs, n_refs, M, Lr, B, 1, self.end_id,
                                     ROUGE_BETA, 0, st["adv"], st["score"], st["counted"])
                else:
                    keys = idf = params = None
                    n_keys = 0
                    if m == "cider-d":
                        keys, idf, params = self.table.device(dev)
                        n_keys = len(self.table)
                        if n_keys == 0:
                            keys = idf = None
                    be.caption_reward(st["fed"], L, st["last"], ids, int(ids.shape[1]), refs, n_refs, M, Lr, keys, idf, n_keys,
                                      params, B, 1, self.end_id, REWARD_KINDS[m], 0, st["adv"], st["score"], st["counted"])
                sums[m].append(st["score"][:, 1].sum())
            count += B
        return {self.log_name(m): float(torch.stack(v).sum().item()) / max(count, 1) if v else 0.0 for m, v in sums.items()}


# ---------------------------------------------------------------------------------------------------- likelihood metrics
def caption_perplexity(model, betas, a0, c0, captions, end_id):
    """Per-token perplexity of the batch's own captions under ``model`` (score_captions): exp(-sum logprob / sum length)
    over the batch; padding is not counted and probabilities are not clipped (unlike the Keras loss test_step reports).
    Returns (perplexity, logprob (B,), length (B,))."""
    lp, length = model.score_captions(betas, a0, c0, captions, end_id=end_id)
    total = int(length.sum())
    ppl = float(np.exp(-float(lp.astype(np.float64).sum()) / total)) if total > 0 else float("nan")
    return ppl, lp, length


def identification(model, betas, a0, c0, captions, end_id, normalise=None, max_rows=None):
    """n-way identification: every scan of the batch scored against all B captions of the batch (the candidate path of
    score_captions with C = B, chunked by ``max_rows``).  Candidate rows with the same ids count as one candidate.
    Returns a dict: scores (B, B) (scores[b, c] = log p(caption c | scan b), length-normalised with normalise="mean"),
    rank (B,) = the number of distinct candidates scoring strictly higher than scan b's own caption, top1 (fraction of
    rank 0) and mrr (mean of 1 / (rank + 1))."""
    caps = np.asarray(captions.detach().cpu().numpy() if hasattr(captions, "detach") else captions)
    if caps.ndim != 2:
        raise ValueError(f"identification takes the batch's captions (B, T), got {caps.shape}")
    B = caps.shape[0]
    cand = np.ascontiguousarray(np.broadcast_to(caps[None], (B,) + caps.shape))
    scores, _ = model.score_captions(betas, a0, c0, cand, end_id=end_id, normalise=normalise, max_rows=max_rows)
    rank = identification_ranks(scores, caps)
    return dict(scores=scores, rank=rank, top1=float((rank == 0).mean()), mrr=float((1.0 / (rank + 1.0)).mean()))


def identification_ranks(scores, captions):
    """rank of candidate b for scan b in a (B, B) score matrix: the number of distinct candidates (rows of ``captions``
    with other ids) scoring strictly higher"""
    caps = np.asarray(captions)
    _, first = np.unique(caps, axis=0, return_index=True)
    keep = np.zeros(len(caps), bool)
    keep[first] = True                                   # one representative per distinct caption
    scores = np.asarray(scores)
    own = scores[np.arange(len(caps)), np.arange(len(caps))]
    return ((scores > own[:, None]) & keep[None, :]).sum(1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- embedding-space retrieval
class SemanticBank:
    """A bank of M known sentence embeddings (M, G) held on the device for nearest-neighbour retrieval in embedding space
    (Model/guse.py: "KNN is used to find a known GUSE vector as the output"): the rows as given and their inverse norms
    1 / sqrt(max(sum x^2, 1e-12)), computed once by tnt_row_inv_norm_f32."""

    def __init__(self, embeddings, device=None):
        import torch
        from . import ops
        e = embeddings if isinstance(embeddings, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(embeddings, np.float32))
        if e.dim() != 2 or e.shape[0] < 1 or e.shape[1] < 1:
            raise ValueError(f"a semantic bank is an (M, G) array of embeddings, got shape {tuple(e.shape)}")
        dev = torch.device(device) if device is not None else (e.device if e.device.type != "cpu" or not torch.cuda.is_available()
                                                                else torch.device("cuda"))
        self.rows = e.to(device=dev, dtype=torch.float32).contiguous()
        self.M, self.G = int(e.shape[0]), int(e.shape[1])
        self.inv = torch.zeros(self.M, dtype=torch.float32, device=dev)
        ops.backend().row_inv_norm(self.rows, self.G, self.inv, self.M, self.G)

    @property
    def device(self):
        return self.rows.device

    def __len__(self):
        return self.M


def semantic_retrieve(model_or_queries, betas, bank, k=5, return_sims=False):
    """The k bank rows nearest in cosine similarity to each query: ``model_or_queries`` a nic.NIC built with semantic= (the
    queries are then model.predict_embedding(betas)) or a (B, G) array of queries (``betas`` is not used).  On the device:
    S = Q bank^T on the model's product route (gemm_sk; the tiled tnt_gemm_f32 without a model), the queries' inverse norms
    (tnt_row_inv_norm_f32) and the selection (tnt_cosine_topk_f32, whose text in include/tnt_hip.h defines the order:
    descending similarity, ties by ascending index, NaN last).  Returns (idx (B, k) int32, sim (B, k) float32) as numpy arrays,
    the only data that crosses the bus; ``return_sims``: also the whole (B, M) similarity matrix, (S * qinv) * binv in
    float32 as the kernel forms it."""
    import torch
    from . import ops
    if not isinstance(bank, SemanticBank):
        raise ValueError(f"bank must be an evaluate.SemanticBank, got {type(bank).__name__}")
    M, G, dev = bank.M, bank.G, bank.device
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(64, M):
        raise ValueError(f"k must be an integer in [1, min(64, M = {M})] (tnt_cosine_topk_f32), got {k!r}")
    k = int(k)
    model = model_or_queries if hasattr(model_or_queries, "predict_embedding") else None
    if model is not None:
        q = model.predict_embedding(betas)
    else:
        q = model_or_queries if isinstance(model_or_queries, torch.Tensor) else torch.as_tensor(
            np.ascontiguousarray(model_or_queries, np.float32))
    q = q.to(device=dev, dtype=torch.float32).contiguous()
    if q.dim() != 2 or q.shape[1] != G or q.shape[0] < 1:
        raise ValueError(f"queries of shape {tuple(q.shape)} against a bank of {G}-wide embeddings")
    B = int(q.shape[0])
    be = ops.backend()
    lds = (M + 3) // 4 * 4
    S = torch.zeros(B, lds, dtype=torch.float32, device=dev)
    if model is not None:
        model.gemm_sk(q, bank.rows, S, B, M, G, G, G, lds, transB=True)
    else:
        be.gemm(q, bank.rows, S, B, M, G, G, G, lds, transB=True)
    qinv = torch.zeros(B, dtype=torch.float32, device=dev)
    be.row_inv_norm(q, G, qinv, B, G)
    idx = torch.zeros(B, k, dtype=torch.int32, device=dev)
    sim = torch.zeros(B, k, dtype=torch.float32, device=dev)
    be.cosine_topk(S, lds, qinv, bank.inv, idx, sim, B, M, k)
    out = (idx.cpu().numpy(), sim.cpu().numpy())
    if return_sims:
        out += (((S[:, :M] * qinv[:, None]) * bank.inv[None, :]).cpu().numpy(),)
    return out


def semantic_ranks(sims, own):
    """rank[b] = the number of bank rows outside own[b] whose similarity is strictly above the best of own[b]; own[b] an
    index or a collection of indices (an image's five captions).  Returns (rank (B,) int64, best (B,) the best own similarity)."""
    sims = np.asarray(sims)
    B, M = sims.shape
    if len(own) != B:
        raise ValueError(f"own holds {len(own)} entries for {B} queries")
    rank, best = np.zeros(B, np.int64), np.zeros(B, sims.dtype)
    for b in range(B):
        mine = np.unique(np.atleast_1d(np.asarray(list(own[b]) if isinstance(own[b], (set, frozenset)) else own[b], np.int64)))
        if mine.size == 0 or mine.min() < 0 or mine.max() >= M:
            raise ValueError(f"own[{b}] must hold at least one bank index in [0, {M}), got {own[b]!r}")
        best[b] = sims[b, mine].max()
        other = np.ones(M, bool)
        other[mine] = False
        rank[b] = int(((sims[b] > best[b]) & other).sum())
    return rank, best


def semantic_identification(model, betas, bank, own):
    """Identification in embedding space, the analysis of the fMRI-decoding literature: the predicted embedding of every scan
    against the whole bank (one product and one selection launch, where evaluate.identification takes B x B decoder passes).
    Returns a dict: rank (B,) (semantic_ranks), top1 / top5 (fraction of rank 0 / rank < 5), mrr (mean of 1 / (rank + 1)),
    mean_cos (mean of each scan's best own similarity) and sims (B, M)."""
    _, _, sims = semantic_retrieve(model, betas, bank, k=1, return_sims=True)
    rank, best = semantic_ranks(sims, own)
    return dict(rank=rank, top1=float((rank == 0).mean()), top5=float((rank < 5).mean()),
                mrr=float((1.0 / (rank + 1.0)).mean()), mean_cos=float(best.astype(np.float64).mean()), sims=sims)
