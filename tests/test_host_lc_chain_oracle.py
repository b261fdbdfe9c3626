"""tests/lc_chain_oracle.py is the float64 truth of tests/test_gpu_attention_paths.py: here its backward is checked
against central finite differences of its forward, so the reference itself can be trusted.  CPU only, no backend."""
import numpy as np

from oracle import ops as O
from lc_chain_oracle import chain_bwd, chain_fwd, chain_masks, out_masks

B, T, R, D, A, U = 3, 3, 5, 4, 4, 8
R_ATTN, R_IN, R_OUT, LW, SEED, STEP = 0.2, 0.3, 0.3, D + 2, 4711, 3
C_MSE = 0.05


def _inputs():
    rng = np.random.default_rng(7)
    n = lambda *s, sc=1.0: rng.standard_normal(s) * sc
    x = dict(F=n(B, R, D), P=n(B, R, A), W2=n(U, A, sc=U ** -0.5), b2=n(A, sc=0.1), v=n(A), bv=n(1),
             xz=n(T, B, U, 4, sc=0.5), Wc=n(D, U, 4, sc=D ** -0.5), Ur=n(U, U, 4, sc=U ** -0.5), zb=n(U, 4, sc=0.1),
             h0=n(B, U, sc=0.5), c0=n(B, U, sc=0.5))
    return x, n(T, B, U)


def test_forward_is_the_per_step_oracles_in_sequence():
    """hs / gates / alpha of chain_fwd are the per-step oracles applied by hand; hd is the one-site-per-step Dropout"""
    x, _ = _inputs()
    masks = chain_masks(T, B, R, D, A, R_ATTN, R_IN, LW, SEED, 16, 48, STEP)
    ko = out_masks(T, B, U, R_OUT, SEED, 77, STEP)
    f = chain_fwd(**x, r_attn=R_ATTN, r_in=R_IN, masks=masks, out_drop=(R_OUT, ko))
    assert f["hs"].shape == (T + 1, B, U) and f["gates"].shape == (T, B, U, 4) and f["alpha"].shape == (T, B, R)
    assert any((~m).any() for m in masks[0]) and any((~m).any() for m in masks[1])      # the masks drop something
    np.testing.assert_allclose(f["alpha"].sum(-1), 1.0, rtol=0, atol=1e-14)
    i, f_, g, o = (f["gates"][1][..., k] for k in range(4))
    c2 = f_ * f["cs"][1] + i * g
    np.testing.assert_allclose(f["cs"][2], c2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(f["hs"][2], o * np.tanh(c2), rtol=0, atol=1e-15)
    (ctx, alpha, _), _ = O.attention_step_fwd(f["hs"][1], x["F"], x["P"], x["W2"], x["b2"], x["v"][:, None], x["bv"],
                                              masks[0][1], R_ATTN)
    np.testing.assert_array_equal(f["alpha"][1], alpha); np.testing.assert_array_equal(f["ctx"][1], ctx)
    scale = 1.0 / (1.0 - np.float64(np.float32(R_IN)))
    np.testing.assert_array_equal(f["ctx_d"][1], np.where(masks[1][1], ctx * scale, 0.0))
    assert np.array_equal(f["hd"] == 0, ~np.stack(ko))


def test_backward_agrees_with_central_differences():
    """chain_bwd against central finite differences of L = sum(w * hs[1:]) + c sum((1 - alpha)^2) through chain_fwd, with
    both dropouts on (fixed masks), for every element of P, F, v, xz and h0 at B=3, T=3, R=5, D=4, A=4, U=8.

    Step h = 1e-6: the truncation error of a central difference is h^2 |L'''| / 6 ~ 1e-12, its rounding error
    eps |L| / h ~ 1e-16 * 10 / 1e-6 = 1e-9 absolute, against gradients of order 0.1 to 1 -- so 1e-7 of a tensor's largest
    gradient is the bound (two decades of margin; an error in the formulas shows at order 1).  Observed worst ratio
    |fd - analytic| / max|analytic| over the five tensors: 1.1e-9 (P; the other four 5.6e-10 .. 9.6e-10)."""
    x, w = _inputs()
    masks = chain_masks(T, B, R, D, A, R_ATTN, R_IN, LW, SEED, 16, 48, STEP)

    def loss(**over):
        f = chain_fwd(**{**x, **over}, r_attn=R_ATTN, r_in=R_IN, masks=masks)
        return (w * f["hs"][1:]).sum() + C_MSE * ((1 - f["alpha"]) ** 2).sum()

    f = chain_fwd(**x, r_attn=R_ATTN, r_in=R_IN, masks=masks)
    g = chain_bwd(x["F"], x["P"], x["W2"], x["v"], x["Wc"], x["Ur"], f["qpre"], f["alpha"], f["gates"], f["cs"], w,
                  r_attn=R_ATTN, r_in=R_IN, masks=masks, alpha_mse_coef=2 * C_MSE)
    analytic = dict(P=g["dP"], F=g["dF"], v=g["dvb"].sum(0), xz=g["dz"], h0=g["dh0"])
    h, worst = 1e-6, {}
    for name, ga in analytic.items():
        fd = np.zeros_like(x[name])
        for idx in np.ndindex(*x[name].shape):
            d = np.zeros_like(x[name]); d[idx] = h
            fd[idx] = (loss(**{name: x[name] + d}) - loss(**{name: x[name] - d})) / (2 * h)
        worst[name] = np.abs(fd - ga).max() / np.abs(ga).max()
    print("worst |fd - analytic| / max|analytic|:", {k: f"{r:.1e}" for k, r in worst.items()})
    assert all(r <= 1e-7 for r in worst.values()), worst


def test_output_dropout_rider_and_float32_mode():
    """out_drop in chain_bwd is Dropout' on dout; dtype=float32 keeps float32 throughout and stays near the float64 result"""
    x, w = _inputs()
    masks = chain_masks(T, B, R, D, A, R_ATTN, R_IN, LW, SEED, 16, 48, STEP)
    ko = out_masks(T, B, U, R_OUT, SEED, 77, STEP)
    f = chain_fwd(**x, r_attn=R_ATTN, r_in=R_IN, masks=masks)
    args = (x["F"], x["P"], x["W2"], x["v"], x["Wc"], x["Ur"], f["qpre"], f["alpha"], f["gates"], f["cs"])
    kw = dict(r_attn=R_ATTN, r_in=R_IN, masks=masks, alpha_mse_coef=0.01)
    a = chain_bwd(*args, w, out_drop=(R_OUT, ko), **kw)
    b = chain_bwd(*args, np.stack([O.dropout_bwd(w[i], ko[i], R_OUT) for i in range(T)]), **kw)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    f32 = chain_fwd(**x, r_attn=R_ATTN, r_in=R_IN, masks=masks, dtype=np.float32)
    b32 = chain_bwd(*args, w, dtype=np.float32, **kw)
    assert all(t.dtype == np.float32 for t in list(f32.values()) + list(b32.values()))
    assert np.abs(f32["hs"] - f["hs"]).max() < 1e-5 and np.abs(f32["hs"] - f["hs"]).max() > 0
