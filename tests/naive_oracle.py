"""Float64 restatement of lc_NIC.call_naive_attention (lc_NIC.py:175-221) -- TEST INFRASTRUCTURE ONLY.

``NaiveLcNIC`` is ``oracle.models.LcNIC`` with the free-running decoder: only the caption's start token is embedded (and
only it gets the text Dropout); every later step is fed the argmax of the step before, with no text Dropout; the output
Dropout acts on the U-wide LSTM output (behind the LSTM-output Dropout), not behind dense_inter; the feature Dropout is
applied a second time behind the encoder.  ``fed_ids`` (B, T) forces the tokens fed to steps 1.. (column 0 is ignored):
float32 and float64 argmaxes may legitimately differ where two logits nearly tie, so a comparison with the device runs
the restatement on the device's fed ids.  No gradient crosses an argmax.

Dropout sites (masks of the Philox stream, oracle/philox.py): text S_TEXT over the logical (B, T, Et) caption tensor,
step 0's rows only; LSTM input S_LSTM_IN + i over (B, 1, D + Et); LSTM output S_LSTM_OUT + i over (B, U); output
S_NOUT + i over (B, U); second feature Dropout S_FEAT2 over (B, R, D).
"""
import numpy as np

from oracle import models as M
from oracle import ops as O

S_FEAT2 = 4
S_NOUT = 144


class NaiveLcNIC(M.LcNIC):

    def forward(self, data, training=False, drop=None, fed_ids=None):
        x, ids, a0, c0 = data
        dt = self.p['lstm/kernel'].dtype
        drop = drop or M.DropCtx(training=training)
        F, enc = self._encode(x.astype(dt), training, drop)
        k_f2 = drop.mask(F.shape, self.r_feat, S_FEAT2)                            # lc_NIC.py:184
        F = O.dropout_fwd(F, k_f2, self.r_feat)
        out, cache = self._decode_fwd(F, ids, a0, c0, training, drop, fed_ids)
        cache['enc'], cache['k_f2'] = enc, k_f2
        return out, cache

    def _decode_fwd(self, F, ids, a0, c0, training, drop, fed_ids=None):
        p = self.p
        dt = p['lstm/kernel'].dtype
        B, T = ids.shape
        U, Et = self.U, self.Et
        E = p['emb_text/embeddings']
        km = drop.mask((B, T, Et), self.r_text, M.S_TEXT)
        k_text = None if km is None else km[:, 0]
        fed = np.zeros((B, T), np.int64)
        fed[:, 0] = ids[:, 0]
        text = O.dropout_fwd(E[fed[:, 0]], k_text, self.r_text)                     # :187-189
        P, Ppre = O.attention_proj_fwd(F, p['attention/W1/kernel'], p['attention/W1/bias'])
        a, c = a0.astype(dt), c0.astype(dt)
        Wl, Ul, bl = p['lstm/kernel'], p['lstm/recurrent_kernel'], p['lstm/bias']
        Wi, bi = p['time_distributed_nonlinear/kernel'], p['time_distributed_nonlinear/bias']
        Wo, bo = p['time_distributed_softmax/kernel'], p['time_distributed_softmax/bias']
        steps, alphas, probs, logits_all, preds, texts = [], [], [], [], np.zeros((B, T), np.int64), []
        for i in range(T):                                                          # :191-219
            k_at = drop.mask((B, self.R, self.A), self.r_attn, M.S_ATTN + i)
            (ctx, alpha, _), acache = O.attention_step_fwd(
                a, F, P, p['attention/W2/kernel'], p['attention/W2/bias'],
                p['attention/V/kernel'], p['attention/V/bias'], k_at, self.r_attn)
            texts.append(text)
            sample = np.concatenate([ctx, text], axis=1)
            k_li = drop.mask((B, 1, sample.shape[1]), self.r_lstm, M.S_LSTM_IN + i)
            sample_d = O.dropout_fwd(sample[:, None, :], k_li, self.r_lstm)[:, 0]
            a, c, lcache = O.lstm_step_fwd(sample_d @ Wl + bl, a, c, Ul)
            k_lo = drop.mask((B, U), self.r_lstm, M.S_LSTM_OUT + i)
            k_no = drop.mask((B, U), self.r_out, S_NOUT + i)
            out = O.dropout_fwd(O.dropout_fwd(a, k_lo, self.r_lstm), k_no, self.r_out)   # :205-207
            inter, ipre = O.dense_fwd(out, Wi, bi, O.ACT_LEAKY)                     # :209
            logits = inter @ Wo + bo                                                # :211
            probs.append(O.softmax(logits))
            logits_all.append(logits)
            preds[:, i] = logits.argmax(axis=-1)                                    # :215
            if i + 1 < T:
                fed[:, i + 1] = preds[:, i] if fed_ids is None else np.asarray(fed_ids)[:, i + 1]
                text = E[fed[:, i + 1]]                                             # :217 (no text Dropout)
            alphas.append(alpha)
            steps.append(dict(acache=acache, sample_d=sample_d, k_li=k_li, lcache=lcache, k_lo=k_lo, k_no=k_no, out=out,
                              inter=inter, ipre=ipre))
        probs = np.stack(probs, axis=1)
        attn = np.stack(alphas, axis=0)[..., None]
        cache = dict(F=F, P=P, Ppre=Ppre, k_text=k_text, steps=steps, fed=fed, preds=preds, text=np.stack(texts, 1),
                     logits=np.stack(logits_all, axis=1))
        return (probs, attn), cache

    def _decode_bwd(self, probs, cache, y_ids):
        p = self.p
        B, T = y_ids.shape
        U, D = self.U, self.D
        g = {}
        dl = np.full((B, T), 1.0 / (B * T), probs.dtype)
        dlogits = O.cce_softmax_bwd(probs, y_ids, dl)
        Wo, Wi = p['time_distributed_softmax/kernel'], p['time_distributed_nonlinear/kernel']
        st = cache['steps']
        inter = np.stack([s['inter'] for s in st], 1)
        g['time_distributed_softmax/kernel'] = (inter.reshape(B * T, -1).T @ dlogits.reshape(B * T, -1)
                                                + 2 * self.l2_out * Wo)
        g['time_distributed_softmax/bias'] = dlogits.sum(axis=(0, 1))
        dinter = dlogits @ Wo.T                                                     # no Dropout on this side
        outs, ipre = np.stack([s['out'] for s in st], 1), np.stack([s['ipre'] for s in st], 1)
        dout, dWi, dbi = O.dense_bwd(outs, Wi, ipre, dinter, O.ACT_LEAKY)
        g['time_distributed_nonlinear/kernel'] = dWi + 2 * self.l2_out * Wi
        g['time_distributed_nonlinear/bias'] = dbi
        Wl, Ul = p['lstm/kernel'], p['lstm/recurrent_kernel']
        W2, v = p['attention/W2/kernel'], p['attention/V/kernel']
        dWl, dUl, dbl = np.zeros_like(Wl), np.zeros_like(Ul), np.zeros_like(p['lstm/bias'])
        dW2, db2 = np.zeros_like(W2), np.zeros_like(p['attention/W2/bias'])
        dv, dbv = np.zeros_like(v), np.zeros_like(p['attention/V/bias'])
        F = cache['F']
        dF, dP = np.zeros_like(F), np.zeros_like(cache['P'])
        dtext = np.zeros((B, T, self.Et), probs.dtype)
        da, dc = np.zeros((B, U), probs.dtype), np.zeros((B, U), probs.dtype)
        for i in reversed(range(T)):
            s = st[i]
            dseq = O.dropout_bwd(O.dropout_bwd(dout[:, i], s['k_no'], self.r_out), s['k_lo'], self.r_lstm)
            dz, dh_prev, dc = O.lstm_step_bwd(da + dseq, dc, s['lcache'], Ul)
            dWl += s['sample_d'].T @ dz
            dUl += s['lcache'][6].T @ dz
            dbl += dz.sum(axis=0)
            dsample = O.dropout_bwd((dz @ Wl.T)[:, None, :], s['k_li'], self.r_lstm)[:, 0]
            dctx, dtext[:, i] = dsample[:, :D], dsample[:, D:]
            dh_att, dF_i, dsum, dW2_i, db2_i, dv_i, dbv_i = O.attention_step_bwd(dctx, F, W2, v, s['acache'])
            dF += dF_i
            dP += dsum
            dW2 += dW2_i
            db2 += db2_i
            dv += dv_i
            dbv += dbv_i
            da = dh_prev + dh_att
        g['lstm/kernel'] = dWl + 2 * self.l2_lstm * Wl
        g['lstm/recurrent_kernel'], g['lstm/bias'] = dUl, dbl
        g['attention/W2/kernel'] = dW2 + 2 * self.l2_attn * W2
        g['attention/W2/bias'] = db2
        g['attention/V/kernel'], g['attention/V/bias'] = dv, dbv
        W1 = p['attention/W1/kernel']
        dF1, dW1, db1 = O.dense_bwd(F, W1, cache['Ppre'], dP, O.ACT_LEAKY)
        dF += dF1
        g['attention/W1/kernel'] = dW1 + 2 * self.l2_attn * W1
        g['attention/W1/bias'] = db1
        dtext[:, 0] = O.dropout_bwd(dtext[:, 0], cache['k_text'], self.r_text)
        rows, flat_ = O.embedding_bwd_rows(dtext, cache['fed'])
        self.last_emb_rows = (rows, flat_)
        g['emb_text/embeddings'] = O.embedding_bwd_dense(dtext, cache['fed'], self.V)
        sparse = {'emb_text/embeddings': np.sqrt((rows * rows).sum())}
        dF = O.dropout_bwd(dF, cache.get('k_f2'), self.r_feat)                     # the second feature Dropout
        return g, sparse, dF

    def train_step(self, data, y_ids, opt, drop=None, fed_ids=None):
        """lc_NIC.train_step on top of call_naive_attention; returns (metrics, gradients, (probs, attn, cache))."""
        drop = drop or M.DropCtx(training=True)
        (probs, attn), cache = self.forward(data, training=True, drop=drop, fed_ids=fed_ids)
        ce, acc, al = self.metrics(probs, attn, y_ids)
        l2 = self.l2_loss()
        grads, sparse = self.backward(probs, cache, y_ids)
        grads, sparse = M.apply_agc(self, grads, sparse)
        opt.apply(self.p, grads, sparse)
        self.p['input_bn/moving_mean'] = cache['enc']['new_mm']
        self.p['input_bn/moving_variance'] = cache['enc']['new_mv']
        for i, dc in enumerate(cache['enc'].get('deep', [])):
            self.p[f'input_bn/deep{i}/moving_mean'], self.p[f'input_bn/deep{i}/moving_variance'] = dc['new_mm'], dc['new_mv']
        return {'loss': ce, 'L2': l2, 'accuracy': acc, 'attention': al, 'lr': opt.lr}, grads, (probs, attn, cache)

    def test_step(self, data, y_ids, fed_ids=None):
        (probs, attn), cache = self.forward(data, training=False, fed_ids=fed_ids)
        ce, acc, al = self.metrics(probs, attn, y_ids)
        return {'loss': ce, 'L2': self.l2_loss(), 'accuracy': acc, 'attention': al}, (probs, attn, cache)
