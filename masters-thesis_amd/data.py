"""Input contract of the hot path: tokeniser, padding, batch generators.

Mirrors what ``AttemptFour/DataLoaders/data_generator_guse.py:129-171`` hands to the model:
``((betas f32 (B,N), cap i32 (B,T), a0 (B,U), c0 (B,U)), target)`` where
``target[:, :-1] = cap[:, 1:]`` (last column 0), one-hot via ``to_categorical`` or -- cheaper,
accepted by every model here -- the int ids themselves.  The NSD files and the lab paths of the
reference are not available (component 8), so the beta loader is a callable and a
synthetic generator with the identical tuple layout is provided for benchmarks.

Host-side staging for wide inputs (full cortex: 327 684 voxels = 84 MB per batch, f1): batches
are assembled in pinned host memory and copied with non_blocking H2D on a side stream,
double-buffered, so the copy of batch i+1 overlaps the step on batch i.
"""
import json
from collections import OrderedDict

import numpy as np
import torch

KERAS_FILTERS = '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n'


class Tokenizer:
    """keras.preprocessing.text.Tokenizer subset used by the reference
    (load_avg_betas.py:184-188: num_words=top_k, oov_token='<unk>', custom filters)."""

    def __init__(self, num_words=None, filters=KERAS_FILTERS, lower=True, split=" ", oov_token=None):
        self.num_words, self.filters, self.lower, self.split, self.oov_token = num_words, filters, lower, split, oov_token
        self.word_counts = OrderedDict()
        self.word_index, self.index_word = {}, {}

    def _seq(self, text):
        if self.lower:
            text = text.lower()
        table = str.maketrans({c: self.split for c in self.filters})
        return [w for w in text.translate(table).split(self.split) if w]

    def fit_on_texts(self, texts):
        for t in texts:
            for w in self._seq(t):
                self.word_counts[w] = self.word_counts.get(w, 0) + 1
        # keras: sort by count descending (stable), OOV token first
        wcounts = sorted(self.word_counts.items(), key=lambda kv: kv[1], reverse=True)
        vocab = ([self.oov_token] if self.oov_token is not None else []) + [w for w, _ in wcounts]
        self.word_index = {w: i + 1 for i, w in enumerate(vocab)}
        self.index_word = {i: w for w, i in self.word_index.items()}

    def texts_to_sequences(self, texts):
        oov = self.word_index.get(self.oov_token) if self.oov_token is not None else None
        out = []
        for t in texts:
            seq = []
            for w in self._seq(t):
                i = self.word_index.get(w)
                if i is not None and (self.num_words is None or i < self.num_words):
                    seq.append(i)
                elif oov is not None:
                    seq.append(oov)
            out.append(seq)
        return out

    def sequences_to_texts(self, seqs):
        return [" ".join(self.index_word.get(int(i), self.oov_token or "") for i in s if int(i) in self.index_word or self.oov_token)
                for s in seqs]

    def to_json(self):
        cfg = dict(num_words=self.num_words, filters=self.filters, lower=self.lower, split=self.split,
                   oov_token=self.oov_token, word_counts=json.dumps(self.word_counts),
                   word_index=json.dumps(self.word_index), index_word=json.dumps(self.index_word))
        return json.dumps({"class_name": "Tokenizer", "config": cfg})


def tokenizer_from_json(s):
    """keras tokenizer_from_json (load_avg_betas.py:136-138): accepts the keras JSON layout."""
    obj = json.loads(s) if isinstance(s, str) else s
    cfg = obj["config"]
    t = Tokenizer(cfg.get("num_words"), cfg.get("filters", KERAS_FILTERS), cfg.get("lower", True), cfg.get("split", " "),
                  cfg.get("oov_token"))
    t.word_counts = OrderedDict(json.loads(cfg.get("word_counts", "{}")))
    t.word_index = json.loads(cfg["word_index"])
    t.index_word = {int(k): v for k, v in json.loads(cfg["index_word"]).items()}
    return t


def pad_sequences(seqs, maxlen, truncating="post", padding="post", value=0, dtype=np.int32):
    """keras pad_sequences as called at data_generator_guse.py:158."""
    out = np.full((len(seqs), maxlen), value, dtype=dtype)
    for i, s in enumerate(seqs):
        s = list(s)
        if len(s) > maxlen:
            s = s[:maxlen] if truncating == "post" else s[-maxlen:]
        if padding == "post":
            out[i, :len(s)] = s
        else:
            out[i, maxlen - len(s):] = s
    return out


def to_categorical(ids, num_classes):
    ids = np.asarray(ids)
    out = np.zeros(ids.shape + (num_classes,), np.float32)
    np.put_along_axis(out, ids[..., None], 1.0, axis=-1)
    return out


def make_target(cap_vector):
    """target[:, :-1] = cap[:, 1:], last column 0 (data_generator_guse.py:161-163)."""
    t = np.zeros_like(cap_vector)
    t[:, :-1] = cap_vector[:, 1:]
    return t


class DataGenerator:
    """keras.utils.Sequence protocol of data_generator_guse.DataGenerator (lines 25-171).
    ``pairs`` rows are (nsd_key, caption, ...); ``load_betas(key, row) -> (N,) float32`` replaces the
    hard-coded np.load of the lab paths (data_generator_guse.py:147-153).  ``load_guse(key, row) -> (G,) float32`` (optional)
    is the caption's sentence embedding, the guse_key column of the reference's batch rows: when given, ``x`` gains it as a
    fifth element (B, G), the target of nic.NIC(semantic=...)."""

    def __init__(self, pairs, batch_size, tokenizer, units, max_len, vocab_size, load_betas, n_voxels, shuffle=True,
                 training=False, one_hot=True, seed=None, load_guse=None):
        self.pairs = np.array(pairs, dtype=object)
        self.batch_size, self.tokenizer, self.units, self.max_len, self.vocab_size = batch_size, tokenizer, units, max_len, vocab_size
        self.load_betas, self.n_voxels, self.load_guse = load_betas, n_voxels, load_guse
        self.shuffle, self.training, self.one_hot = shuffle, training, one_hot
        self.rng = np.random.default_rng(seed)
        self.on_epoch_end()

    def __len__(self):
        return len(self.pairs) // self.batch_size

    def on_epoch_end(self):
        if self.shuffle:
            self.rng.shuffle(self.pairs)

    def __getitem__(self, index):
        batch = self.pairs[index * self.batch_size:(index + 1) * self.batch_size]
        B = len(batch)
        betas = np.zeros((B, self.n_voxels), np.float32)
        for i, row in enumerate(batch):
            betas[i] = self.load_betas(row[0], row)
        cap = pad_sequences(self.tokenizer.texts_to_sequences([r[1] for r in batch]), self.max_len)
        target = make_target(cap)
        if self.one_hot:
            target = to_categorical(target, self.vocab_size)
        init = np.zeros((B, self.units), np.float32)
        x = (betas, cap, init, init.copy())
        if self.load_guse is not None:
            x += (np.stack([np.asarray(self.load_guse(r[0], r), np.float32) for r in batch]),)
        return (x, target) if self.training else (x, target, np.array([r[0] for r in batch]))


class SyntheticGenerator:
    """Synthetic batches with the reference's tuple layout: betas ~ N(0,1) (the reference's
    betas are z-scored per voxel), captions = <start>, 6..13 tokens uniform in [3, V), <end>, zero
    padding.  ``device`` set: tensors are created once on the device (benchmarks).  ``guse_dim`` = G: a fifth input (B, G),
    unit-norm Gaussian rows from a generator of their own seeded with (seed, index), so that every other array of a batch
    keeps its bits."""

    def __init__(self, n_batches, batch_size, n_voxels, units, max_len, vocab_size, seed=42, one_hot=False, device=None,
                 guse_dim=None):
        self.n, self.B, self.N, self.U, self.T, self.V = n_batches, batch_size, n_voxels, units, max_len, vocab_size
        self.seed, self.one_hot, self.device = seed, one_hot, device
        if guse_dim is not None and (isinstance(guse_dim, bool) or int(guse_dim) != guse_dim or guse_dim < 1):
            raise ValueError(f"guse_dim must be None or an integer >= 1, got {guse_dim!r}")
        self.guse_dim = None if guse_dim is None else int(guse_dim)
        self._cache = {}

    def __len__(self):
        return self.n

    def on_epoch_end(self):
        pass

    def __getitem__(self, index):
        if index in self._cache:
            return self._cache[index]
        rng = np.random.default_rng(self.seed + index)
        x = rng.standard_normal((self.B, self.N)).astype(np.float32)
        cap = np.zeros((self.B, self.T), np.int32)
        for b in range(self.B):
            hi = max(1, self.T - 2)
            L = int(rng.integers(min(6, hi), min(13, hi) + 1))
            cap[b, 0] = 1
            cap[b, 1:1 + L] = rng.integers(3, self.V, size=L)
            cap[b, 1 + L] = 2
        tgt = make_target(cap)
        z = np.zeros((self.B, self.U), np.float32)
        item = ((x, cap, z, z.copy()), to_categorical(tgt, self.V) if self.one_hot else tgt)
        if self.guse_dim is not None:
            g = np.random.default_rng([self.seed, index]).standard_normal((self.B, self.guse_dim))
            g = (g / np.sqrt((g * g).sum(axis=1, keepdims=True))).astype(np.float32)
            item = (item[0] + (g,), item[1])
        if self.device is not None:
            dev = lambda a: torch.as_tensor(a).to(self.device)
            item = (tuple(dev(a) for a in item[0]), dev(item[1]))
            self._cache[index] = item
        return item


class PinnedPrefetcher:
    """Double-buffered host->device staging for wide batches: wraps any generator; batch i+1 is fetched from the
    generator and copied H2D on a side stream BY A WORKER THREAD while the model steps on batch i (at full-cortex width
    moving an 84 MB batch takes longer than the GPU step, so none of it may sit on the launching thread).
    Arrays the generator hands over in pinned memory (torch pinned tensors or numpy views of them) are DMA-ed
    asynchronously from where they are -- a generator that does so must not rewrite such an array before two more
    batches have been requested; pageable arrays go through the runtime's own staged copy, on the worker thread
    (measured on MI355X, tools/full_cortex_bench.py: a private pageable->pinned memcpy is 5x slower than that).
    ``betas_dtype="float16"``: the betas cross PCIe as IEEE half (half the bytes of the tensor that dominates the
    transfer) and are widened by the staging kernel (tnt_stage_batch_h16); an opt-in approximation (10-bit mantissa on
    z-scored betas), off by default so that results match the reference.  It pays when the generator already yields
    float16 (a dataset stored that way); a float32 source is converted on the worker thread, which costs more than
    the bytes save."""

    def __init__(self, generator, device, betas_dtype="float32", threaded=True):
        assert betas_dtype in ("float32", "float16")
        self.betas_dtype = np.float16 if betas_dtype == "float16" else np.float32
        self.gen, self.device = generator, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._next = None
        # two slots of persistent device buffers.  Batch i lives in slot i & 1 from its copy until batch i + 2 is staged:
        # a slot is overwritten only after the compute stream has consumed the batch it held (an event recorded on the
        # compute stream when the NEXT batch is requested); the host keeps the source arrays of a slot alive until the
        # slot's asynchronous copy has completed.
        self._dev = [None, None]
        self._h2d = [None, None]
        self._src = [None, None]
        self._pool = None
        if threaded and self.stream is not None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="tnt-prefetch")

    def __len__(self):
        return len(self.gen)

    def on_epoch_end(self):
        self._drain()
        self.gen.on_epoch_end()
        self._next = None

    def _drain(self):
        if self._next is not None and hasattr(self._next[1], "result"):
            self._next[1].result()

    def _stage(self, index, slot, consumed=None):
        (x, cap, a0, c0), tgt = self.gen[index][:2]
        ts = [a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a)) for a in (x, cap, a0, c0, tgt)]
        want0 = torch.float16 if self.betas_dtype is np.float16 else torch.float32
        if ts[0].dtype != want0:
            ts[0] = ts[0].to(want0)
        if self.stream is None:
            return tuple(ts), None
        torch.cuda.set_device(self.device)
        if self._h2d[slot] is not None:
            self._h2d[slot].synchronize()            # the previous copy into this slot is done: its sources may go
        if self._dev[slot] is None or any(d.shape != t.shape or d.dtype != t.dtype for d, t in zip(self._dev[slot], ts)):
            self._dev[slot] = [torch.empty(t.shape, dtype=t.dtype, device=self.device) for t in ts]
        with torch.cuda.stream(self.stream):
            if consumed is not None:
                self.stream.wait_event(consumed)     # the batch this slot held has been read by the compute stream
            for src, dv in zip(ts, self._dev[slot]):
                dv.copy_(src, non_blocking=True)     # pinned source: asynchronous DMA; pageable: the runtime's staged copy
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._h2d[slot], self._src[slot] = ev, ts
        return tuple(self._dev[slot]), ev

    def _submit(self, index, consumed):
        if self._pool is None:
            return self._stage(index, index & 1, consumed)
        return self._pool.submit(self._stage, index, index & 1, consumed)

    def __getitem__(self, index):
        consumed = None
        if self.stream is not None:
            # everything the compute stream has been given so far -- the step on the previous batch included -- precedes this
            consumed = torch.cuda.Event()
            consumed.record(torch.cuda.current_stream())
        if self._next is None or self._next[0] != index:
            self._drain()
            self._next = (index, self._submit(index, consumed))
        staged = self._next[1]
        if hasattr(staged, "result"):
            staged = staged.result()
        (x, cap, a0, c0, tgt), ev = staged
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
        nxt = index + 1
        self._next = (nxt, self._submit(nxt, consumed)) if nxt < len(self.gen) else None
        return ((x, cap, a0, c0), tgt)


TOKEN_WEIGHT_SCHEMES = ("inverse", "inverse_sqrt", "effective")


def token_class_weights(captions, vocab_size, scheme="inverse_sqrt", beta=0.999, pad_weight=0.0, clip=None, mean_one=True):
    """Class weights for ``CategoricalCrossentropy(class_weight=...)`` / ``fit(class_weight=...)`` from the integer caption
    array of a corpus (any shape; id 0 is the padding): frequent words weigh less, so that "a", "of", "man" do not dominate
    the words that carry a scan's content.  With n_v the number of occurrences of id v:
      "inverse"       1 / n_v
      "inverse_sqrt"  1 / sqrt(n_v)
      "effective"     (1 - beta) / (1 - beta^n_v)     (Cui et al. 2019, class-balanced loss; 0 < beta < 1)
    A class that never occurs gets the weight of n_v = 1.  ``mean_one``: the weights of the ids 1 .. V-1 are scaled so that
    their mean over the corpus's non-padding tokens, sum_v n_v w_v / sum_v n_v, is 1 -- the loss scale, and so the learning
    rate, stay comparable with the unweighted loss.  ``clip`` = (lo, hi): those weights are then clipped to [lo, hi] (in the
    scaled units; the mean is not restored).  ``w[0] = pad_weight`` last.  float64 inside, float32 out, deterministic."""
    V = int(vocab_size)
    if V < 1:
        raise ValueError(f"vocab_size must be >= 1, got {vocab_size!r}")
    if scheme not in TOKEN_WEIGHT_SCHEMES:
        raise ValueError(f"scheme must be one of {TOKEN_WEIGHT_SCHEMES}, got {scheme!r}")
    ids = np.asarray(captions)
    if ids.dtype.kind not in "iu":
        raise ValueError(f"captions must be an integer array, got dtype {ids.dtype}")
    ids = ids.reshape(-1).astype(np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= V):
        raise ValueError(f"captions hold ids outside [0, {V})")
    pad = float(pad_weight)
    if not 0.0 <= pad < float("inf"):
        raise ValueError(f"pad_weight must be finite and >= 0, got {pad_weight!r}")
    count = np.bincount(ids, minlength=V).astype(np.float64)
    n = np.maximum(count, 1.0)
    if scheme == "inverse":
        w = 1.0 / n
    elif scheme == "inverse_sqrt":
        w = 1.0 / np.sqrt(n)
    else:
        b = float(beta)
        if not 0.0 < b < 1.0:
            raise ValueError(f"beta must be in (0, 1), got {beta!r}")
        w = (1.0 - b) / -np.expm1(n * np.log(b))
    if mean_one:
        tokens = count[1:].sum()
        if tokens > 0:
            w = w * (tokens / (count[1:] * w[1:]).sum())
    if clip is not None:
        lo, hi = (float(c) for c in clip)
        if not 0.0 <= lo <= hi < float("inf"):
            raise ValueError(f"clip must be (lo, hi) with 0 <= lo <= hi, both finite, got {clip!r}")
        w = np.clip(w, lo, hi)
    w[0] = pad
    return w.astype(np.float32)
