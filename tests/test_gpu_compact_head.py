"""The vocabulary head over the distinct caption rows only (nic.NIC ``compact_head``): the row map built by the staging
launch, the device-side live extent of tnt_gemm3_f32 / tnt_gemm3_pair_f32, the persistent LSTM chains addressed through the
map, the weighted softmax-CCE, and the training step with compaction on against off and against the float64 oracle."""
import numpy as np
import pytest
import torch

from oracle import models as M

pytestmark = pytest.mark.gpu

POISON = 5.0


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, want, rtol, atol=None):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return
    scale = np.abs(want).max() + 1e-30
    atol = rtol * scale if atol is None else atol
    err = np.abs(got - want).max()
    print(f"max abs err {err:.3e} bound {atol:.3e}")
    assert err <= atol, f"max abs err {err:.3e} > {atol:.3e} (scale {scale:.3e})"


@pytest.fixture(scope="module")
def be():
    import masters_thesis_amd.ops as ops
    return ops.backend()


def r4(n):
    return (n + 3) // 4 * 4


def word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


G3_TOL = lambda K: 1e-6 * max(1.0, (K / 256) ** 0.5)         # the bound of test_gpu_ops.py::test_gemm3*
TILE_BM = {1: 160, 5: 64, 7: 64}


# ------------------------------------------------------------------------------ gemm3: live rows of M
@pytest.mark.parametrize("tile", [7, 5, 1])
def test_gemm3_live_rows_of_m(be, tile):
    """NN at M=200, N=96, K=72 with the bias rider: rows below the live word are the product, rows at or past it keep the
    value written beforehand; live 0 leaves C alone; a null word and a word holding M give the same bits."""
    from masters_thesis_amd.ops import LIVE_ROWS_M
    Mr, N, K = 200, 96, 72
    rng = np.random.default_rng(tile)
    lda, ldb, ldc = r4(K), r4(N), r4(N) + 4
    A = np.zeros((Mr, lda)); A[:, :K] = rng.standard_normal((Mr, K))
    Bm = np.zeros((K, ldb)); Bm[:, :N] = rng.standard_normal((K, N))
    bias = rng.standard_normal(N)
    want = A[:, :K] @ Bm[:, :N] + bias
    Ad, Bd, bd = dev(A), dev(Bm), dev(bias)
    ref = torch.full((Mr, ldc), POISON, device="cuda")
    be.gemm3(Ad, Bd, ref, Mr, N, K, lda, ldb, ldc, bias=bd, tile=tile)
    bm = TILE_BM[tile]
    for live in (0, 1, bm - 1, bm, bm + 1, Mr, Mr + 7):
        lv = min(live, Mr)
        C = torch.full((Mr, ldc), POISON, device="cuda")
        be.gemm3(Ad, Bd, C, Mr, N, K, lda, ldb, ldc, bias=bd, tile=tile, live=word(live), live_mode=LIVE_ROWS_M)
        close(C[:lv, :N], want[:lv], rtol=G3_TOL(K))
        assert torch.equal(C[:lv], ref[:lv]), ("live rows differ from the unbounded launch", tile, live)
        assert torch.equal(C[lv:], torch.full((Mr - lv, ldc), POISON, device="cuda")), ("row past live written", tile, live)
        assert torch.equal(C[:, N:], torch.full((Mr, ldc - N), POISON, device="cuda"))


@pytest.mark.parametrize("tile", [7, 1])
def test_gemm3_live_rows_of_m_nt_split(be, tile):
    """NT with the K split reduced in the launch (K=1200, two splits): every split of a dead tile leaves together, the
    exchange buffer stays armed, live rows equal the unbounded launch bit for bit."""
    from masters_thesis_amd.ops import LIVE_ROWS_M
    Mr, N, K, S = 200, 96, 1200, 2
    rng = np.random.default_rng(10 + tile)
    lda, ldb, ldc = r4(K), r4(K), r4(N) + 4
    A = rng.standard_normal((Mr, lda)); Bm = rng.standard_normal((N, ldb))
    want = A @ Bm.T
    Ad, Bd = dev(A), dev(Bm)
    wf = be.gemm3_work_floats(Mr, N, tile, S)
    assert wf > 0
    work = torch.empty(r4(wf), device="cuda")
    be.gemm3_work_arm(work)
    armed = work.view(torch.int32).clone()
    sync = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = torch.full((Mr, ldc), POISON, device="cuda")
    be.gemm3(Ad, Bd, ref, Mr, N, K, lda, ldb, ldc, transB=True, tile=tile, splitk=S, work=work, sync=sync)
    bm = TILE_BM[tile]
    for live in (0, 1, bm - 1, bm, bm + 1, Mr):
        C = torch.full((Mr, ldc), POISON, device="cuda")
        be.gemm3(Ad, Bd, C, Mr, N, K, lda, ldb, ldc, transB=True, tile=tile, splitk=S, work=work, sync=sync,
                 live=word(live), live_mode=LIVE_ROWS_M)
        torch.cuda.synchronize()
        assert torch.equal(work.view(torch.int32), armed), ("exchange buffer not re-armed", tile, live)
        close(C[:live, :N], want[:live], rtol=G3_TOL(K))
        assert torch.equal(C[:live], ref[:live])
        assert torch.equal(C[live:], torch.full((Mr - live, ldc), POISON, device="cuda")), ("row past live written", tile, live)
    assert int(sync.sum()) == 0


# ------------------------------------------------------------------------------ gemm3: live rows of K
@pytest.mark.parametrize("tile", [7, 5, 1])
def test_gemm3_live_rows_of_k(be, tile):
    """TN with the column-sum rider at M=200, N=96, K=72: the sums run over k < live (0: the empty sum), whatever the rows
    past it hold (NaN here); a split is refused; null word == word holding K, bit for bit."""
    from masters_thesis_amd.ops import LIVE_ROWS_K
    from masters_thesis_amd._lib import KernelLibraryError
    Mr, N, K = 200, 96, 72
    rng = np.random.default_rng(20 + tile)
    lda, ldb, ldc = r4(Mr), r4(N), r4(N) + 4
    A = rng.standard_normal((K, lda)); Bm = np.zeros((K, ldb)); Bm[:, :N] = rng.standard_normal((K, N))
    Ad, Bd = dev(A), dev(Bm)
    ref, refcol = torch.full((Mr, ldc), POISON, device="cuda"), torch.full((ldc,), POISON, device="cuda")
    be.gemm3(Ad, Bd, ref, Mr, N, K, lda, ldb, ldc, transA=True, colsum=refcol, tile=tile)
    bm = TILE_BM[tile]
    for live in (0, 1, 31, 32, 33, bm - 1, bm, bm + 1, K):
        lv = min(live, K)
        An, Bn = Ad.clone(), Bd.clone()
        An[lv:] = float("nan"); Bn[lv:] = float("nan")              # rows past the live extent are never multiplied
        C, col = torch.full((Mr, ldc), POISON, device="cuda"), torch.full((ldc,), POISON, device="cuda")
        be.gemm3(An, Bn, C, Mr, N, K, lda, ldb, ldc, transA=True, colsum=col, tile=tile, live=word(live), live_mode=LIVE_ROWS_K)
        close(C[:, :N], A[:lv, :Mr].T @ Bm[:lv, :N], rtol=G3_TOL(K), atol=None if lv else 0.0)
        close(col[:N], Bm[:lv, :N].sum(0), rtol=0, atol=2e-6 * np.abs(Bm[:lv, :N]).sum(0).max())
        assert torch.equal(C[:, N:], torch.full((Mr, ldc - N), POISON, device="cuda"))
        assert torch.equal(col[N:], torch.full((ldc - N,), POISON, device="cuda"))
        if lv == K:
            assert torch.equal(C, ref) and torch.equal(col, refcol), ("word == K differs from the unbounded launch", tile)
    work = torch.empty(r4(max(be.gemm3_work_floats(Mr, N, tile, 2), 4)), device="cuda")
    be.gemm3_work_arm(work)
    with pytest.raises(KernelLibraryError):
        be.gemm3(Ad, Bd, torch.empty((Mr, ldc), device="cuda"), Mr, N, K, lda, ldb, ldc, transA=True, tile=tile, splitk=2,
                 work=work, sync=torch.zeros(1, dtype=torch.int32, device="cuda"), live=word(5), live_mode=LIVE_ROWS_K)
    with pytest.raises(KernelLibraryError):       # rows of M of a transposed A, rows of K of an NN product: no such form
        be.gemm3(Ad, Bd, torch.empty((Mr, ldc), device="cuda"), Mr, N, K, lda, ldb, ldc, transA=True, tile=tile,
                 live=word(5), live_mode=1)


@pytest.mark.parametrize("t1,t2,S2", [(5, 7, 1), (7, 5, 2), (4, 7, 1)])
def test_gemm3_pair_shares_one_live_word(be, t1, t2, S2):
    """The head's gradient pair in one launch, both products bounded by ONE word: dW = Out^T dlogits and db over the live
    rows, dOut = dlogits W^T for the live rows (the others keep their poison)."""
    from masters_thesis_amd.ops import LIVE_ROWS_M, LIVE_ROWS_K
    R, U, V = 200, 64, 96
    rng = np.random.default_rng(30 + t1 + t2)
    ldV = r4(V)
    Out = rng.standard_normal((R, U)); dlog = np.zeros((R, ldV)); dlog[:, :V] = rng.standard_normal((R, V))
    W = np.zeros((U, ldV)); W[:, :V] = rng.standard_normal((U, V))
    Od, Dd, Wd = dev(Out), dev(dlog), dev(W)
    assert be.gemm3_pair_supported(t1, True, False, t2, False, True)
    wf = r4(be.gemm3_work_floats(R, U, t2, S2)) if S2 > 1 else 0
    work = torch.empty(max(wf, 4), device="cuda")
    be.gemm3_work_arm(work)
    sync = torch.zeros(1, dtype=torch.int32, device="cuda")
    for live in (0, 1, 63, 64, 65, 160, R):
        lw = word(live)
        On, Dn = Od.clone(), Dd.clone()
        On[live:] = float("nan"); Dn[live:] = float("nan")
        dW, db = torch.full((U, ldV), POISON, device="cuda"), torch.full((ldV,), POISON, device="cuda")
        dO = torch.full((R, U), POISON, device="cuda")
        d1 = be.gemm3_desc(On, Dn, dW, U, V, R, U, ldV, ldV, transA=True, colsum=db, tile=t1, live=lw, live_mode=LIVE_ROWS_K)
        d2 = be.gemm3_desc(Dn, Wd, dO, R, U, V, ldV, ldV, U, transB=True, tile=t2, splitk=S2, work=work if S2 > 1 else None,
                           sync=sync if S2 > 1 else None, live=lw, live_mode=LIVE_ROWS_M)
        be.gemm3_pair(d1, d2)
        close(dW[:, :V], Out[:live].T @ dlog[:live, :V], rtol=G3_TOL(R), atol=None if live else 0.0)
        close(db[:V], dlog[:live, :V].sum(0), rtol=0, atol=2e-6 * max(np.abs(dlog[:live, :V]).sum(0).max(), 1e-30) if live else 0.0)
        close(dO[:live], dlog[:live, :V] @ W[:, :V].T, rtol=G3_TOL(V))
        assert torch.equal(dO[live:], torch.full((R - live, U), POISON, device="cuda")), ("dOut row past live written", live)
    assert int(sync.sum()) == 0


# ------------------------------------------------------------------------------ row map, chains, softmax
B8, T6, U512, V37 = 8, 6, 512, 37


def hand_caps():
    """full length, minimal (<start>, <end>, 0 ...), every length in between, and a fed 0 whose target is not the carried one"""
    cap = np.array([[1, 3, 4, 5, 6, 2],
                    [1, 2, 0, 0, 0, 0],
                    [1, 7, 2, 0, 0, 0],
                    [1, 8, 9, 2, 0, 0],
                    [1, 10, 11, 12, 2, 0],
                    [1, 2, 0, 0, 0, 0],
                    [1, 13, 14, 15, 16, 17],
                    [1, 5, 0, 7, 2, 0]], np.int32)
    tgt = np.zeros_like(cap)
    tgt[:, :-1] = cap[:, 1:]
    return cap, tgt


def ref_map(cap, tgt):
    """(pos [T*B], weight [rows], compact target [rows], group of every position) by the definition in include/tnt_hip.h"""
    B, T = cap.shape
    has = np.zeros((T, B), bool)
    group = np.zeros((T, B), np.int64)                 # time-major index of the position whose row (t, b) shares
    for b in range(B):
        rep = None
        for t in range(T):
            merged = t > 0 and cap[b, t] == 0 and tgt[b, t] == tgt[b, rep]
            if not merged:
                rep = t
                has[t, b] = True
            group[t, b] = rep * B + b
    pos = np.full(T * B, -1, np.int64)
    pos[has.reshape(-1)] = np.arange(int(has.sum()))
    rows = int(has.sum())
    w = np.zeros(rows)
    for g in group.reshape(-1):
        w[pos[g]] += 1
    tc = np.zeros(rows, np.int64)
    tt = tgt.T.reshape(-1)
    tc[pos[pos >= 0]] = tt[pos >= 0]
    return pos, w, tc, group.reshape(-1)


def stage_map(be, cap, tgt):
    B, T = cap.shape
    n, N = B * T, 4
    x, z = torch.zeros(B, N, device="cuda"), torch.zeros(B, U512, device="cuda")
    xd, h0, c0 = torch.empty(B, N, device="cuda"), torch.empty(B, U512, device="cuda"), torch.empty(B, U512, device="cuda")
    capd, tgtd = torch.empty(B, T, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    pos = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w, tc = torch.full((n,), POISON, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    live = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lr, cr = torch.full((n,), POISON, device="cuda"), torch.full((n,), POISON, device="cuda")
    be.stage_batch_map(x, xd, dev(cap, torch.int32), capd, dev(tgt, torch.int32), tgtd, z, h0, z, c0, B, T, N, N, U512,
                       pos, w, tc, live, lr, cr)
    return pos, w, tc, live, lr, cr, capd, tgtd


def test_row_map(be):
    cap, tgt = hand_caps()
    pos, w, tc, live, lr, cr, capd, tgtd = stage_map(be, cap, tgt)
    rp, rw, rt, _ = ref_map(cap, tgt)
    rows = len(rw)
    assert rows == 6 + 2 + 3 + 4 + 5 + 2 + 6 + 5 and int(live.item()) == rows
    assert np.array_equal(pos.cpu().numpy(), rp)
    assert np.array_equal(w.cpu().numpy()[:rows], rw) and np.array_equal(tc.cpu().numpy()[:rows], rt)
    for t_ in (w, tc, lr, cr):
        assert not t_[rows:].any(), "rows past live must be zeroed"
    assert torch.equal(lr[:rows], torch.full((rows,), POISON, device="cuda"))
    assert np.array_equal(capd.cpu().numpy(), cap) and np.array_equal(tgtd.cpu().numpy(), tgt.T.reshape(-1))
    assert w.sum().item() == B8 * T6
    # every caption at full length: the identity map
    full = np.tile(np.array([[1, 3, 4, 5, 6, 2]], np.int32), (B8, 1))
    ft = np.zeros_like(full); ft[:, :-1] = full[:, 1:]
    pos, w, tc, live, *_ = stage_map(be, full, ft)
    assert int(live.item()) == B8 * T6 and np.array_equal(pos.cpu().numpy(), np.arange(B8 * T6)) and bool((w == 1).all())


@pytest.mark.parametrize("B,T", [(64, 15), (70, 15), (300, 5)])
def test_row_map_sizes(be, B, T):
    """random padded captions at the benchmark's size (the map held in LDS), just past that limit (B*T = 1050: worked on in
    global memory) and with more captions than the workgroup has threads; some interior zeros"""
    rng = np.random.default_rng(B + T)
    cap = np.zeros((B, T), np.int32)
    for b in range(B):
        L = int(rng.integers(0, T - 1))
        cap[b, 0] = 1
        cap[b, 1:1 + L] = rng.integers(3, 50, size=L)
        cap[b, 1 + L] = 2
        if L >= 2 and rng.random() < 0.3:
            cap[b, 1 + int(rng.integers(0, L))] = 0
    tgt = np.zeros_like(cap); tgt[:, :-1] = cap[:, 1:]
    pos, w, tc, live, lr, cr, *_ = stage_map(be, cap, tgt)
    rp, rw, rt, _ = ref_map(cap, tgt)
    rows = len(rw)
    assert int(live.item()) == rows and np.array_equal(pos.cpu().numpy(), rp)
    assert np.array_equal(w.cpu().numpy()[:rows], rw) and np.array_equal(tc.cpu().numpy()[:rows], rt)
    for t_ in (w, tc, lr, cr):
        assert not t_[rows:].any()


@pytest.fixture(scope="module")
def chain(be):
    """one position-ordered and one compacted run of both chains on the hand-built captions, shared by the tests below"""
    if not be.lstm_seq_supported(B8, U512):
        pytest.skip("persistent LSTM kernel not supported on this device")
    B, T, U, S = B8, T6, U512, T6 + 1
    rng = np.random.default_rng(5)
    cap, tgt = hand_caps()
    pos, w, tc, live, *_ = stage_map(be, cap, tgt)
    rp, rw, rt, group = ref_map(cap, tgt)
    xz = dev(rng.standard_normal((S, B, U, 4)) * 0.5)
    Ur = dev(rng.standard_normal((U, U, 4)) / np.sqrt(U))
    bl = dev(rng.standard_normal((U, 4)) * 0.1)
    capd = dev(cap, torch.int32)
    sync = torch.zeros(1025, dtype=torch.int32, device="cuda")
    guard = torch.zeros(1, device="cuda")

    def fwd(p):
        hs, cs = torch.zeros(S + 1, B, U, device="cuda"), torch.zeros(S + 1, B, U, device="cuda")
        out, gates = torch.full((T * B, U), POISON, device="cuda"), torch.empty(S, B, U, 4, device="cuda")
        be.lstm_seq_fwd(xz, hs, cs, Ur, bl, capd, T, 1, out, gates, S, B, U, sync, guard, out_pos=p)
        return out, gates, hs, cs
    out_p, gates, hs, cs = fwd(None)
    out_c, gates_c, hs_c, cs_c = fwd(pos)
    assert torch.equal(gates, gates_c) and torch.equal(hs, hs_c) and torch.equal(cs, cs_c)
    dout_p = rng.standard_normal((T * B, U))
    dout_c = np.zeros((T * B, U))
    np.add.at(dout_c, rp[group], dout_p)                 # a row's gradient: the sum over the positions that share it
    work = torch.empty(be.lstm_seq_bwd_work_floats(B, U), device="cuda")

    def bwd(d, p):
        dz = torch.empty(S, B, U, 4, device="cuda")
        be.lstm_seq_bwd(Ur, dev(d).view(T, B, U), capd, T, 1, gates, cs, dz, work, S, B, U, sync, guard, dout_pos=p)
        return dz
    dz_p, dz_c = bwd(dout_p, None), bwd(dout_c, pos)
    ident = torch.arange(T * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert int(sync[1024].item()) == 0 and guard.item() == 0.0
    return dict(pos=pos, w=w, tc=tc, live=live, rp=rp, rw=rw, rt=rt, group=group, out_p=out_p, out_c=out_c, dz_p=dz_p, dz_c=dz_c,
                fwd=fwd, bwd=bwd, dout_p=dout_p, ident=ident, tgt=tgt)


def test_forward_chain_writes_compacted_rows(chain):
    rp, rows = chain["rp"], len(chain["rw"])
    has = torch.tensor(rp >= 0, device="cuda")
    idx = torch.tensor(rp[rp >= 0], device="cuda")
    assert torch.equal(chain["out_c"][idx], chain["out_p"][has]), "compacted rows != position-ordered rows"
    # a merged position holds the row of its group in the position-ordered run (the carried output)
    assert torch.equal(chain["out_p"], chain["out_c"][torch.tensor(rp[chain["group"]], device="cuda")])
    assert torch.equal(chain["out_c"][rows:], torch.full((B8 * T6 - rows, U512), POISON, device="cuda")), "row past live written"
    # the identity map is the call without a map
    out_i, *_ = chain["fwd"](chain["ident"])
    assert torch.equal(out_i, chain["out_p"])


def test_backward_chain_reads_compacted_rows(chain):
    """dZ with the gradient rows summed per group and read through the map, against the position-ordered run.  The two differ
    in the order of at most T = 6 float32 additions into the carried output gradient (relative 6 * 2^-24 = 4e-7 of the sum)
    carried through 7 linear steps of O(1) gain: bound 1e-5 of max |dZ|."""
    close(chain["dz_c"], chain["dz_p"].cpu().double().numpy(), rtol=1e-5)
    dz_i = chain["bwd"](chain["dout_p"], chain["ident"])
    assert torch.equal(dz_i, chain["dz_p"]), "identity map differs from the call without a map"


def test_weighted_softmax_over_live_rows(be, chain):
    """loss / accuracy sums and dlogits of the distinct rows times their multiplicity against the position-ordered head"""
    n, V, ldV = B8 * T6, V37, r4(V37)
    rows, rp, group = len(chain["rw"]), chain["rp"], chain["group"]
    rng = np.random.default_rng(6)
    W = dev(np.pad(rng.standard_normal((U512, V)) * 0.2, ((0, 0), (0, ldV - V))))
    logits_p = chain["out_p"] @ W
    logits_c = torch.full((n, ldV), POISON, device="cuda")
    logits_c[:rows] = chain["out_c"][:rows] @ W
    tgt_p = dev(chain["tgt"].T.reshape(-1), torch.int32)
    lp, cp, dp = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, ldV, device="cuda")
    be.softmax_cce(logits_p, tgt_p, None, lp, cp, dp, n, V, ldV, 1.0 / n)
    lc, cc = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    dc = logits_c.clone()
    be.softmax_cce_live(logits_c, chain["tc"], None, lc, cc, dc, n, V, ldV, 1.0 / n, chain["live"], chain["w"])
    # float64 reference of the weighted rows
    x = logits_c[:rows, :V].cpu().double().numpy()
    p = np.exp(x - x.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    y = chain["rt"]
    want_l = -np.log(np.clip(p[np.arange(rows), y], 1e-7, 1 - 1e-7)) * chain["rw"]
    oh = np.zeros_like(p); oh[np.arange(rows), y] = 1
    close(lc[:rows], want_l, rtol=1e-4)               # float64 truth: the 1e-4 of test_gpu_ops.py
    close(dc[:rows, :V], (p - oh) * chain["rw"][:, None] / n, rtol=1e-4)
    assert np.array_equal(cc[:rows].cpu().numpy(), (p.argmax(1) == y) * chain["rw"])
    assert torch.equal(dc[rows:], logits_c[rows:]) and not lc[rows:].any() and not cc[rows:].any(), "row past live touched"
    # ... and against the position-ordered launch: same totals, a row's gradient = the sum over its positions
    assert abs(lc.sum().item() - lp.sum().item()) <= 1e-5 * abs(lp.sum().item())
    assert cc.sum().item() == cp.sum().item()
    dsum = torch.zeros(n, ldV, device="cuda", dtype=torch.float64)
    dsum.index_add_(0, torch.tensor(rp[group], device="cuda"), dp.double())
    close(dc[:rows, :V], dsum[:rows, :V].cpu().numpy(), rtol=1e-5)
    # unit weights over all rows == the plain entry point, bit for bit
    one, full = torch.ones(n, device="cuda"), torch.tensor([n], dtype=torch.int32, device="cuda")
    l1, c1, d1 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, ldV, device="cuda")
    be.softmax_cce_live(logits_p, tgt_p, None, l1, c1, d1, n, V, ldV, 1.0 / n, full, one)
    assert torch.equal(l1, lp) and torch.equal(c1, cp) and torch.equal(d1, dp)


# ------------------------------------------------------------------------------ the training step
NV = 256


def make_model(compact, rates=(0.0, 0.0, 0.0), **kw):
    from masters_thesis_amd.nic import NIC
    from masters_thesis_amd.optimizers import Adam
    m = NIC(NV, U512, U512, V37, T6, *rates, 0.01, 0.00003, 0.00001, seed=42, **kw)
    m.compact_head = compact
    m.compile(Adam(learning_rate=1e-4, beta_1=0.9, beta_2=0.98, epsilon=1e-8, clipnorm=0.1))
    return m


def dev_batch(rng, cap, tgt):
    x = rng.standard_normal((B8, NV)).astype(np.float32)
    z = np.zeros((B8, U512), np.float32)
    host = ((x, cap, z, z.copy()), tgt)
    d = ((dev(x), dev(cap, torch.int32), dev(z), dev(z)), dev(tgt, torch.int32))
    return host, d


def took_compact(m):
    return ("train", B8, T6, "compact") in m._graphs


def test_training_compaction_on_against_off():
    """three training steps, dropout on, compaction on against off: the bounds
    test_persistent_lstm_forward_trains_like_the_step_kernels holds two kernel families to."""
    rng = np.random.default_rng(9)
    cap, tgt = hand_caps()
    _, batch = dev_batch(rng, cap, tgt)
    a, b = make_model(True, rates=(0.0, 0.2, 0.2)), make_model(False, rates=(0.0, 0.2, 0.2))
    ha = [a.train_step(batch).as_floats() for _ in range(3)]
    hb = [b.train_step(batch).as_floats() for _ in range(3)]
    if not a._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    assert took_compact(a) and not took_compact(b)
    a.check_device_errors(); b.check_device_errors()
    for x, y in zip(ha, hb):
        print(x, y)
        assert abs(x["loss"] - y["loss"]) <= 2e-5 * abs(y["loss"]), (x, y)
        assert abs(x["accuracy"] - y["accuracy"]) <= 2.0 / (B8 * T6)
    wa, wb = a.get_weights_dict(), b.get_weights_dict()
    for k in wa:
        d = np.abs(wa[k] - wb[k])
        print(k, d.max(), (d > 3e-5).mean())
        assert (d > 3e-5).mean() <= 5e-3, (k, d.max(), (d > 3e-5).mean())


def test_compacted_step_gradients_match_oracle():
    """one step's loss, accuracy and EVERY gradient against the float64 oracle: |err| <= 1e-4 max|g| + 1e-10 per tensor (the
    rule of test_gpu_fullsize.py::test_train_step_matches_oracle_at_full_size)"""
    rng = np.random.default_rng(21)
    cap, tgt = hand_caps()
    host, batch = dev_batch(rng, cap, tgt)
    rates = (0.0, 0.0, 0.0)
    model = make_model(True, rates)
    orc = M.NICDense(NV, U512, U512, V37, T6, *rates, 0.01, 0.00003, 0.00001)
    orc.p = {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()}
    names = [k for k in orc.p if "moving_" not in k]
    lam = {k: model.arena.entries[k].l2 for k in names}
    w0 = {k: v.copy() for k, v in orc.p.items()}
    opt = M.AdamState({k: orc.p[k] for k in names}, lr=1e-4, b1=0.9, b2=0.98, eps=1e-8, clipnorm=0.1)
    res, grads, _ = orc.train_step(host[0], host[1], opt, M.DropCtx(seed=model.seed, step=0, training=True))
    got = model.train_step(batch).as_floats()
    if not model._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    assert took_compact(model)
    model.check_device_errors()
    for k in ("loss", "accuracy"):
        tol = 1e-6 if k == "accuracy" else 1e-4 * abs(res[k]) + 1e-7
        print(k, got[k], res[k])
        assert abs(got[k] - res[k]) <= tol, (k, got[k], res[k])
    for k in names:
        if grads.get(k) is None:
            continue
        gm = model.get_gradient(k).astype(np.float64) + 2 * lam[k] * w0[k]
        scale, err = np.abs(grads[k]).max(), np.abs(gm - grads[k]).max()
        print(k, err, scale)
        assert err <= 1e-4 * scale + 1e-10, (k, err, scale)


def test_full_length_captions_are_bit_identical_and_plan_equals_graph():
    """every caption at full length: live = T*B, unit weights, the identity map -- the step is bit-identical with compaction
    on and off.  And on the hand-built captions the recorded launch plan and the hipGraph replay the same bits."""
    rng = np.random.default_rng(3)
    full = np.tile(np.array([[1, 3, 4, 5, 6, 2]], np.int32), (B8, 1))
    full[:, 1:5] = rng.integers(3, V37, size=(B8, 4))
    ft = np.zeros_like(full); ft[:, :-1] = full[:, 1:]
    _, batch = dev_batch(rng, full, ft)
    a, b = make_model(True, rates=(0.0, 0.2, 0.2)), make_model(False, rates=(0.0, 0.2, 0.2))
    # the compacted head forward is always a gemm3 product; without compaction a product this small (V = 37) goes to the
    # generic tiled kernel, another summation order.  Same kernel family on both sides: no size threshold.
    a.g3_min_flops = b.g3_min_flops = 0.0
    ha = [a.train_step(batch).as_floats() for _ in range(4)]
    hb = [b.train_step(batch).as_floats() for _ in range(4)]
    if not a._seq_lstm:
        pytest.skip("persistent LSTM kernel not supported on this device")
    assert took_compact(a) and int(a.head_live.item()) == B8 * T6
    assert ha == hb
    wa, wb = a.get_weights_dict(), b.get_weights_dict()
    assert all(np.array_equal(wa[k], wb[k]) for k in wa)
    cap, tgt = hand_caps()
    _, batch = dev_batch(rng, cap, tgt)
    p, g = make_model(True, rates=(0.0, 0.2, 0.2)), make_model(True, rates=(0.0, 0.2, 0.2))
    g.plan_step = False
    hp = [p.train_step(batch).as_floats() for _ in range(5)]
    hg = [g.train_step(batch).as_floats() for _ in range(5)]
    assert took_compact(p) and took_compact(g) and isinstance(p._graphs[("train", B8, T6, "compact")], tuple)
    assert hp == hg
    wp, wg = p.get_weights_dict(), g.get_weights_dict()
    assert all(np.array_equal(wp[k], wg[k]) for k in wp)
    p.check_device_errors(); g.check_device_errors()
