"""Input contract, tokenizer, callbacks, config.yaml and the fit loop (CPU, mock backend)."""
import json
import os

import numpy as np
import pytest
import yaml

import masters_thesis_amd.ops as ops
from masters_thesis_amd import data as D, callbacks as CB, config as CFG
from mock_backend import MockBackend

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def mock_backend():
    old = ops._backend
    ops.set_backend(MockBackend())
    yield
    ops.set_backend(old)


def caps():
    # data fixture held by the reference: soloist/Modified-Show-And-Tell-Keras/target_caps.txt (first 40 lines)
    with open(os.path.join(HERE, "golden", "target_caps_head40.txt")) as f:
        # the corpus itself contains the literal token <unk>; keras then lets the later index win over the
        # reserved OOV slot, which is not what this test is about -> substitute it
        return [l.strip().replace("<unk>", "thing") for l in f if l.strip()]


def test_tokenizer_keras_semantics():
    texts = ["<start> " + c + " <end>" for c in caps()]
    # filters of load_avg_betas.py:186 ('<' and '>' are not filtered, so <start>/<end>/<pad>/<unk> survive)
    tok = D.Tokenizer(num_words=50, oov_token="<unk>", filters='!"#$%&()*+.,-/:;=?@[\\]^_`{|}~\t\n ')
    tok.fit_on_texts(texts)
    assert tok.word_index["<unk>"] == 1
    counts = sorted(tok.word_counts.values(), reverse=True)
    by_index = [tok.word_counts[tok.index_word[i]] for i in range(2, 2 + len(counts))]
    assert by_index == counts                                    # index order == count order
    seqs = tok.texts_to_sequences(texts[:5])
    assert all(all(0 < i < 50 for i in s) for s in seqs)         # num_words cap, OOV -> 1
    assert seqs[0][0] == tok.word_index["<start>"] and seqs[0][-1] == tok.word_index["<end>"]
    tok2 = D.tokenizer_from_json(tok.to_json())
    assert tok2.texts_to_sequences(texts[:5]) == seqs
    cap = D.pad_sequences(seqs, 8)
    assert cap.shape == (5, 8) and cap.dtype == np.int32
    tgt = D.make_target(cap)
    assert np.array_equal(tgt[:, :-1], cap[:, 1:]) and (tgt[:, -1] == 0).all()
    oh = D.to_categorical(tgt, 50)
    assert oh.shape == (5, 8, 50) and np.array_equal(oh.argmax(-1), tgt)


def test_data_generator_tuple_layout():
    texts = caps()
    tok = D.Tokenizer(num_words=30, oov_token="<unk>")
    tok.fit_on_texts(texts)
    pairs = [(i, "<start> " + t + " <end>") for i, t in enumerate(texts[:20])]
    rng = np.random.default_rng(0)
    table = rng.standard_normal((20, 33)).astype(np.float32)
    gen = D.DataGenerator(pairs, 4, tok, 16, 9, 30, lambda key, row: table[int(key)], 33, shuffle=False, training=True)
    assert len(gen) == 5
    (betas, cap, a0, c0), target = gen[1]
    assert betas.shape == (4, 33) and np.array_equal(betas, table[4:8])
    assert cap.shape == (4, 9) and a0.shape == (4, 16) and not a0.any() and target.shape == (4, 9, 30)
    gen2 = D.DataGenerator(pairs, 4, tok, 16, 9, 30, lambda key, row: table[int(key)], 33, shuffle=False, training=False)
    assert len(gen2[0]) == 3                                     # (+ nsd_key) as data_generator_guse.py:170-171


def test_config_yaml_fit_callbacks(tmp_path):
    cfg = dict(run="t", log="./Log/", seed=42, epochs=2, batch_size=4, max_length=6, top_k=20, optimizer="Adam",
               alpha=0.0001, clipnorm=0.1, decay=0, dropout_input=0, dropout_features=0.2, dropout_text=0.2,
               dropout_lstm=0.2, dropout_attn=0.2, dropout_out=0.2, input_reg=0.01, attn_reg=0.001, lstm_reg=0.00003,
               output_reg=0.00001, units=16, attn_units=8, group_size=16, embedding_features=512, embedding_text=12)
    p = tmp_path / "config.yaml"
    p.write_text(yaml.dump(cfg))
    config = CFG.load_config(str(p))
    from helpers import tiny_groups
    groups = (tiny_groups(40, 4, np.random.default_rng(1)), [config["group_size"]] * 4)
    model = CFG.build_model(config, groups, device="cpu")
    assert model.optimizer.lr == 1e-4 and model.optimizer.clipnorm == 0.1
    train = D.SyntheticGenerator(3, 4, 40, 16, 6, 21, seed=1, one_hot=True)
    val = D.SyntheticGenerator(2, 4, 40, 16, 6, 21, seed=9)
    hist_csv = str(tmp_path / "loss_history.csv")
    cbs = [CB.LossHistory(hist_csv), CB.LearningRateScheduler(lambda e: 1e-3 if e == 0 else 5e-4),
           CB.ModelCheckpoint(str(tmp_path / "model" / "model-ep{epoch:03d}.npz"), monitor="val_loss", save_best_only=False)]
    hist = model.fit(train, epochs=2, steps_per_epoch=3, batch_size=4, callbacks=cbs, validation_data=val,
                     validation_steps=2, initial_epoch=0, verbose=0)
    assert len(hist["loss"]) == 2 and "val_loss" in hist and "attention" in hist
    assert model.optimizer.lr == 5e-4
    assert os.path.exists(tmp_path / "model" / "model-ep002.npz")
    rows = open(hist_csv).read().strip().splitlines()
    assert len(rows) == 1 + 2 * (3 + 2)
    m2 = CFG.build_model(config, groups, device="cpu")
    m2.load_weights(str(tmp_path / "model" / "model-ep002.npz"), by_name=True, skip_mismatch=True)
    for k in model.keras_shapes:
        assert np.array_equal(m2.get_weight(k), model.get_weight(k)), k


def test_bleu_known_answers():
    """sentence_bleu restates nltk's published algorithm (ThinkAndTell/img_evaluate.py:245-248 calls it with
    SmoothingFunction().method1).  Known answers: the worked example of the nltk documentation and closed forms."""
    from masters_thesis_amd.evaluate import sentence_bleu, bleu_scores
    hyp1 = "It is a guide to action which ensures that the military always obeys the commands of the party".split()
    ref1 = "It is a guide to action that ensures that the military will forever heed Party commands".split()
    ref2 = ("It is the guiding principle which guarantees the military forces always being under the command of "
            "the Party").split()
    ref3 = "It is the practical guide for the army always to heed the directions of the party".split()
    assert abs(sentence_bleu([ref1, ref2, ref3], hyp1, smoothing=None) - 0.5045666840058485) < 1e-12
    assert sentence_bleu([ref1], ref1) == pytest.approx(1.0)
    assert sentence_bleu([["a", "b"]], ["c", "d"]) == 0.0
    # one matching unigram of two, no bigram: p1 = 1/2, p2 = eps/1 with method 1; without smoothing 0
    assert sentence_bleu([["a", "b", "c"]], ["a", "x"], weights=(0.5, 0.5), smoothing=None) == 0.0
    import math
    want = math.exp(1 - 3 / 2) * math.exp(0.5 * math.log(0.5) + 0.5 * math.log(0.1))
    assert sentence_bleu([["a", "b", "c"]], ["a", "x"], weights=(0.5, 0.5)) == pytest.approx(want)
    b = bleu_scores([ref1, ref2, ref3], hyp1)
    assert len(b) == 4 and b[0] > b[1] > b[2] > b[3] > 0


def test_eval_dumps_have_the_reference_layouts(tmp_path):
    """eval.py:148-216: output_captions / output_captions_raw / attention_scores .npy + tokenizer.json."""
    from masters_thesis_amd import evaluate as EV
    from masters_thesis_amd.lc_nic import NIC
    from masters_thesis_amd.fc_nic import NICfc
    from helpers import tiny_groups
    B, N, T, V, U, R, Dg = 3, 40, 5, 21, 16, 4, 16
    tok = D_tok()
    cfg = dict(max_length=T, units=U)
    gen = D.SyntheticGenerator(2, B, N, U, T, V, seed=3)
    groups = (tiny_groups(N, R, np.random.default_rng(1)), [Dg] * R)
    model = NIC(groups, U, 512, 12, 8, V, T, 0, 0, 0, 0, 0, 0, 0.01, 0.001, 3e-5, 1e-5, device="cpu")
    outs, attn = EV.eval_model(model, gen, tok, cfg, str(tmp_path), 7)
    assert outs.shape == (2 * B, T, 1) and attn.shape == (2 * B, T, R, 1)
    assert np.load(tmp_path / "output_captions_7.npy").shape == (2 * B, T, 1)
    assert np.load(tmp_path / "output_captions_raw_7.npy").shape == (2 * B, T, V)
    assert np.load(tmp_path / "attention_scores_7.npy").shape == (2 * B, T, R, 1)
    tok2 = D.tokenizer_from_json(open(tmp_path / "tokenizer.json").read())
    assert tok2.word_index == tok.word_index
    fc = NICfc(N, U, 12, 12, V, T, 0, 0, 0, 0, 0, 0.01, 3e-5, 1e-5, device="cpu")
    ids = EV.eval_fc_model(fc, gen, tok, cfg, str(tmp_path / "fc"), 2)
    assert ids.shape == (2 * B, T, 1) and np.load(tmp_path / "fc" / "output_captions_2.npy").shape == (2 * B, T, 1)
    caps = EV.ids_to_captions(np.array([[[1], [5], [6], [2], [7]], [[5], [0], [0], [0], [0]]]), tok)
    assert caps == [[tok.index_word[5], tok.index_word[6]], [tok.index_word[5]]]


def D_tok():
    tok = D.Tokenizer(num_words=20, oov_token="<unk>", filters='!"#$%&()*+.,-/:;=?@[\\]^_`{|}~ ')
    tok.fit_on_texts(["<start> a man rides a horse <end>", "<start> a dog runs on the beach <end>"])
    tok.word_index["<pad>"] = 0
    tok.index_word[0] = "<pad>"
    # ids used by the test: 1 = <start>? make them explicit
    tok.word_index.update({"<start>": 1, "<end>": 2})
    tok.index_word.update({1: "<start>", 2: "<end>"})
    return tok


# data fixture held by the reference: soloist/Modified-Show-And-Tell-Keras/target_caps.txt (all 4 000 lines)
REF_CAPS = os.path.join(HERE, "golden", "target_caps.txt")


def test_tokenizer_pipeline_over_the_reference_corpus():
    """The only caption corpus the reference holds (4 000 lines, stored as a fixture) through the whole text side of the input
    contract: build_tokenizer (load_avg_betas.py:184-188: fit, then '<pad>' -> 0), create_pairs' '<start> ... <end>'
    wrapping (:259-265), texts_to_sequences / pad_sequences / shifted target / to_categorical
    (data_generator_guse.py:156-163).  Asserted: the invariants those call sites rely on, and the vocabulary against an
    independent derivation (collections.Counter)."""
    from collections import Counter
    with open(REF_CAPS) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == 4000
    texts = ["<start> " + " ".join(w.lower() for w in l.replace(".", " ").replace(",", " ").split(" ") if w) + " <end>" for l in lines]
    top_k, max_len = 1000, 13
    filters = '!"#$%&()*+.,-/:;=?@[\\]^_`{|}~\t\n '
    tok = D.Tokenizer(num_words=top_k, oov_token="<unk>", filters=filters)
    tok.fit_on_texts(texts)
    # independent vocabulary: words by count (ties by first occurrence), the OOV token in slot 1; the corpus contains the
    # literal token '<unk>', and keras' dict(zip(...)) lets its later (count-ranked) index win over the reserved slot
    cnt = Counter(w for t in texts for w in t.split(" "))
    assert dict(tok.word_counts) == dict(cnt)
    ranked = ["<unk>"] + [w for w, _ in sorted(cnt.items(), key=lambda kv: -kv[1])]
    want = {}
    for i, w in enumerate(ranked):
        want[w] = i + 1
    assert tok.word_index == want
    assert "<unk>" in cnt and tok.word_index["<unk>"] > 1 and 1 not in tok.index_word
    assert cnt["<start>"] == 4000 <= cnt["<end>"] and tok.word_index["<end>"] < tok.word_index["<start>"] < 8   # the corpus holds literal <end> tokens too
    # load_avg_betas.py:187-188
    tok.word_index["<pad>"] = 0
    tok.index_word[0] = "<pad>"
    seqs = tok.texts_to_sequences(texts)
    assert len(seqs) == 4000
    flat = np.concatenate([np.asarray(s) for s in seqs])
    assert flat.min() == 0 and flat.max() < top_k                                # num_words cut-off; '<pad>' -> 0
    n_rare = sum(c for w, c in cnt.items() if want[w] >= top_k)
    oov = tok.word_index["<unk>"]                                                # keras: word_index.get(oov_token) -- here NOT 1
    assert oov < top_k and not (flat == 1).any()
    assert n_rare > 0 and int((flat == oov).sum()) == n_rare + cnt["<unk>"]      # every cut-off word became the OOV id
    for t, s in zip(texts[:200], seqs[:200]):
        ws = t.split(" ")
        assert len(s) == len(ws) and s[0] == tok.word_index["<start>"] and s[-1] == tok.word_index["<end>"]
        assert all((i == 0) == (w == "<pad>") for w, i in zip(ws, s))
    cap = D.pad_sequences(seqs, max_len)                                         # truncating='post', padding='post'
    assert cap.shape == (4000, max_len) and cap.dtype == np.int32
    for s, row in zip(seqs, cap):
        k = min(len(s), max_len)
        assert list(row[:k]) == s[:k] and not row[k:].any()
    tgt = D.make_target(cap)
    assert np.array_equal(tgt[:, :-1], cap[:, 1:]) and not tgt[:, -1].any()
    oh = D.to_categorical(tgt[:64], top_k)
    assert oh.shape == (64, max_len, top_k) and oh.dtype == np.float32
    assert np.array_equal(oh.argmax(-1), tgt[:64]) and np.array_equal(oh.sum(-1), np.ones((64, max_len), np.float32))
    tok2 = D.tokenizer_from_json(tok.to_json())                                  # load_tokenizer(), :136-138
    assert tok2.word_index == tok.word_index and tok2.texts_to_sequences(texts) == seqs
    assert tok2.sequences_to_texts([seqs[0]])[0].split(" ")[0] == "<start>"
