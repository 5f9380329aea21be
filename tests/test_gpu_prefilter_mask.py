"""The pre-filtered corpus search over live rows and per-query filters on the MI355X: gdr_sim_topk_prefilter_masked
with GDR_SIM_LIVE_MASK and with GDR_SIM_QUERY_MASK, gdr_prefilter_update_rows, ops.PrefilteredCorpus(masks=True) and
GDRRetriever(search_prefilter=True).

Every raw result is held to three oracles: no disallowed row is returned; the float64 restatement (tests/live_ref.py) under the
project's parity rule (TOL, oracle/parity_rules.py); and BIT EQUALITY of values and ids with gdr_sim_topk_prefilter over the compacted
operands D[allowed], D16[allowed] with the same dnorm_max, ids mapped back — the rescoring of a row depends on (q, row, d) alone and the
select is exact.  A flagged list (status 1) is the top-k of a subset and would escape all three, so every shape x mask pair is first
shown NOT to flag, on the host: make_plan, prefilter_survivor_factor and eps2 (csrc/sim_topk.hip) are restated below in numpy over the
bf16-rounded operands, and the candidate list and the band are asserted to fit before the device is asked (occupancy()).  The
restatement is also what tests/test_prefilter_mask_host.py holds against the library's size function."""
import math
import types

import numpy as np
import pytest
import torch

import expand_ref
import lifecycle_ref
import live_ref
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import order_insensitive_topk_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr
from live_ref import mask_bytes
from sim_widths import in_sample_tile, plan

TOL = 1e-4                         # oracle/parity_rules.py: |got - ref| <= 1e-4 + 1e-4 |ref|, ids exact beyond twice that
LIVE, QM = _ffi.SIM_LIVE_MASK, _ffi.SIM_QUERY_MASK
CNT_STRIDE = 32

# name -> (B, N, d, k).  d = 64: the tiled bf16 GEMM core at every B; d = 256 at B <= 32: the bf16 stream kernels
SHAPES = {
    "sampled_B40": (40, 20_000, 64, 10),                            # tiled core, stride 39
    "sampled_B4": (4, 20_000, 64, 10),
    "stream_B4": (4, 20_000, 256, 10),                              # bf16 stream kernels
    "ragged_B4": (4, 20_011, 64, 10),
    "stride1_B4": (4, 1_000, 64, 10),                               # no filter pass
    "k100_B40": (40, 20_000, 64, 100),                              # stride 13
}
STRIDE = {"stride1_B4": 1, "k100_B40": 13}                          # every other shape: 39
MASKS = ("none", "topk_union", "inside_sample_tiles", "outside_sample_tiles", "word_boundaries", "q0_top200_dead")
REFUSED_FLAGS = (0, LIVE | QM, LIVE | _ffi.SIM_EXHAUSTIVE, QM | _ffi.SIM_EXHAUSTIVE, LIVE | _ffi.SIM_NO_STREAM, QM | _ffi.SIM_NO_STREAM,
                 QM | _ffi.SIM_ROW_GATHER, QM | _ffi.SIM_ROW_GATHER | _ffi.sim_gather_chunks(2), LIVE | _ffi.sim_gather_chunks(1),
                 _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM, _ffi.SIM_ROW_GATHER, 32, LIVE | 32)


# ------------------------------------------------------------------------- csrc/sim_topk.hip restated (host only, no library call)
def _up(n, a=256):
    return -(-n // a) * a


def make_plan(B, N, k, survivors=1.0):
    """make_plan(B, N, k, exhaustive = false, survivors): sample stride, sample slots, list capacity (sim_widths.plan), bytes."""
    stride, n_slots, cap = plan(N, k, survivors=survivors)
    total = 2 * _up(B * cap * 4) + _up(B * CNT_STRIDE * 4) + _up(B * 4) + (_up(B * 16 * 128 * 8) if B <= 32 else 0)
    return types.SimpleNamespace(stride=stride, n_slots=n_slots, cap=cap, total=total)


def survivor_factor(N, d, k):
    """prefilter_survivor_factor: by how much the threshold lowered by 2 eps_q admits more rows than the sample's k-th score."""
    p0 = make_plan(1, N, k)
    if p0.stride == 1:
        return 1.0
    Qf = lambda z: 0.5 * math.erfc(z * 0.70710678118654752)   # noqa: E731
    tail = float(k) / float(p0.n_slots)
    lo, hi = -8.0, 8.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if Qf(mid) > tail:
            lo = mid
        else:
            hi = mid
    zl = 0.5 * (lo + hi)
    dz = 2.0 * math.sqrt(float(d)) * (2.0 ** -7 + 2.0 ** -16 + d * 2.0 ** -22) * 1.25
    return max(0.5 * Qf(zl - dz) / tail, 1.0)


def prefilter_plan(B, N, d, k):
    """make_prefilter_plan: the list plan, the band capacity cap2 and the bytes of one call's own layout."""
    p = make_plan(B, N, k, survivor_factor(N, d, k))
    cap2 = 1024
    while cap2 < 4 * k:
        cap2 *= 2
    p.cap2 = cap2
    p.total += _up(B * d * 2) + _up(B * 4)
    return p


def eps2(Q, dnorm_max, d):
    """sim_qprep_kernel's 2 eps_q per query (float64 here; the kernel's fp32 rounding is inside occupancy()'s slack)."""
    nq = np.linalg.norm(np.asarray(Q, np.float64), axis=1) * 1.0001
    return 2.0 * nq * float(dnorm_max) * (2.0 ** -7 + 2.0 ** -16 + d * 2.0 ** -22) * 1.01


def occupancy(S16, allowed, Q, dnorm_max, d, k):
    """What the masked call's lists will hold, from the fp64 scores S16 [B, N] of the bf16-rounded operands and allowed bool [B, N]:
    (longest candidate list, its capacity, fullest band, its capacity, queries without k allowed sample rows).  The kernel's scores
    are fp32 sums of the same exact products: they differ from S16 by at most d 2^-24 |q| |row| 1.01 each, so every cut below is
    lowered by `slack` = four times that bound — the counts are upper bounds of what the device can see."""
    B, N = S16.shape
    p = prefilter_plan(B, N, d, k)
    inside = in_sample_tile(N, p.stride)
    e2 = eps2(Q, dnorm_max, d)
    slack = 4.0 * d * 2.0 ** -24 * np.linalg.norm(np.asarray(Q, np.float64), axis=1) * float(dnorm_max) * 1.01
    longest = fullest = 0
    no_thr = []
    for q in range(B):
        a, s = allowed[q], S16[q]
        samp = np.sort(s[inside & a])[::-1]
        if p.stride > 1:
            if samp.size < k:
                no_thr.append(q)
                thr = -np.inf
            else:
                thr = samp[k - 1] - e2[q] - slack[q]
            listed = inside | (s >= thr)
            longest = max(longest, p.n_slots + int((~inside & (s >= thr)).sum()))     # disallowed survivors take slots too
        else:
            listed = inside
            longest = max(longest, p.n_slots)
        mine = np.sort(s[listed & a])[::-1]
        if mine.size:
            kth = mine[min(k, mine.size) - 1]
            fullest = max(fullest, int((mine >= kth - e2[q] - 2 * slack[q]).sum()))
    return longest, p.cap, fullest, p.cap2, no_thr


def assert_cannot_flag(s, allowed, what):
    """The condition of every exactness case: list and band fit with room to spare, and the sample gives every query a threshold."""
    longest, cap, fullest, cap2, no_thr = occupancy(s.S16, allowed, s.Q, s.dnorm, s.d, s.k)
    assert not no_thr or s.stride == 1, f"{what}: queries {no_thr} have fewer than k allowed sample rows"
    assert longest <= cap and fullest <= cap2, f"{what}: list {longest} of {cap}, band {fullest} of {cap2}: the case could flag"
    return longest, fullest


# ------------------------------------------------------------------------------------------------ data (host), made once per shape
_HOST, _DATA = {}, {}


def host_data(name):
    """Operands as tests/test_gpu_live_search.py builds them, with two planted exact-tie rows for each of the first two queries; the
    fp64 scores of the fp32 operands (S: what the answer ranks) and of the bf16-rounded operands (S16: what the pre-filter sees)."""
    if name not in _HOST:
        B, N, d, k = SHAPES[name]
        D = synth.make_corpus(N, d, seed=N + d)
        Q, _ = synth.make_queries(D, B, seed=B + d)
        for q in range(min(B, 2)):
            src = np.argsort(-(D @ Q[q]))[:2]
            D[(src + 777) % N] = D[src]
        Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
        S = live_ref.scores(Q, D)
        S16 = live_ref.scores(Qt.bfloat16().double().numpy(), Dt.bfloat16().double().numpy())
        dnorm = float(np.sqrt((D.astype(np.float64) ** 2).sum(1).max())) * (1.0 + 1e-6)
        ref_top = live_ref.topk(S, np.ones(N, bool), max(k, 200))[1]
        _HOST[name] = types.SimpleNamespace(name=name, B=B, N=N, d=d, k=k, Q=Q, D=D, Qt=Qt, Dt=Dt, S=S, S16=S16, dnorm=dnorm,
                                            ref_top=ref_top, stride=prefilter_plan(B, N, d, k).stride)
    return _HOST[name]


def live_mask(s, name, top=None, seed=0, q=0):
    """bool [N] for the live flag (and, with seed / q, one query's bitmap of a per-query variant).  top: the ids of the unfiltered
    answer that must die under topk_union (default: the fp64 reference's, every query's)."""
    rng = np.random.default_rng(len(name) + s.N + 1000 * seed)
    live = np.ones(s.N, bool)
    inside = in_sample_tile(s.N, s.stride)
    if top is None:
        top = np.unique(s.ref_top[:, :s.k])
    if name == "topk_union":
        live[top] = False
    elif name == "inside_sample_tiles":
        live[inside & (rng.random(s.N) < 0.5)] = False
    elif name == "outside_sample_tiles":
        live[~inside & (rng.random(s.N) < 0.3)] = False
    elif name == "word_boundaries":
        live[:32] = False
        live[-33:] = False
    elif name == "q0_top200_dead":                                            # a band from the UNMASKED k-th score would be too narrow
        live[s.ref_top[q, :200]] = False
    return live


def query_masks(s, name, top=None):
    """bool [B, N], a different bitmap per query: query 0 allows everything, query 1 has ITS best 200 rows dead, the others draw the
    named mask independently ("none": independent random halves; topk_union: the query's own unfiltered answer).  stride1_B4: query 2
    allows nothing and query 3 seven rows."""
    a = np.ones((s.B, s.N), bool)
    a[1] = live_mask(s, "q0_top200_dead", q=1)
    for q in range(2, s.B):
        if name == "none":
            a[q] = np.random.default_rng(s.N + s.B + q).random(s.N) < 0.5
        elif name == "topk_union":
            a[q] = live_mask(s, name, top=s.ref_top[q, :s.k] if top is None else top[q])
        else:
            a[q] = live_mask(s, name, seed=q, q=q)
    if s.name == "stride1_B4":
        a[2] = False
        a[3] = False
        a[3, [0, 31, 32, 500, 777, 998, 999]] = True
    return a


# ------------------------------------------------------------------------------------------------------------------- device side
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


def _data(name, dev):
    if name not in _DATA:
        s = types.SimpleNamespace(**vars(host_data(name)))
        s.Qd, s.Dd = s.Qt.to(dev), s.Dt.to(dev)
        s.P = ops.PrefilteredCorpus(s.Dd)
        assert torch.equal(s.P.D16.cpu(), s.Dt.bfloat16()) and abs(s.P.dnorm_max - s.dnorm) <= 1e-5 * s.dnorm
        s.v0, s.i0, st0 = _plain(s.Qd, s.Dd, s.P.D16, s.P.dnorm_max, s.k)
        assert int(st0.abs().sum()) == 0
        _DATA[name] = s
    return _DATA[name]


def _out(B, k, device):
    return (torch.empty((B, k), dtype=torch.float32, device=device), torch.empty((B, k), dtype=torch.int32, device=device),
            torch.empty((B,), dtype=torch.int32, device=device))


def _plain(Qd, Dd, D16, dnorm, k, idx_offset=0):
    """gdr_sim_topk_prefilter with a workspace of exactly the declared size."""
    B, d = Qd.shape
    N = Dd.shape[0]
    need = lib().gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k)
    ws = torch.empty(need, dtype=torch.uint8, device=Qd.device)
    v, i, st = _out(B, k, Qd.device)
    rc = lib().gdr_sim_topk_prefilter(ptr(Qd), B, ptr(Dd), ptr(D16), dnorm, N, d, k, idx_offset, ptr(v), ptr(i), ptr(st), ptr(ws), need,
                                      stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return v, i, st


def _fill(ws, B, N, live=None, allowed=None):
    """The bitmap(s) at the head of the workspace: live bool [N], or allowed bool [B, N] with bitmap q at byte q * M."""
    if live is not None:
        words = torch.from_numpy(live_ref.pack(live)).to(ws.device)
        ws[:words.numel() * 4].view(torch.int32).copy_(words)
    else:
        M, W = mask_bytes(N), (N + 31) // 32
        words = torch.from_numpy(np.stack([live_ref.pack(a) for a in allowed])).to(ws.device)
        ws[:B * M].view(torch.int32).view(B, M // 4)[:, :W].copy_(words)


def _masked(s, live=None, allowed=None, idx_offset=0):
    """gdr_sim_topk_prefilter_masked with a workspace of exactly the declared size."""
    flags = LIVE if live is not None else QM
    need = lib().gdr_sim_topk_prefilter_masked_workspace_bytes(s.B, s.N, s.d, s.k, flags)
    assert need == (1 if live is not None else s.B) * mask_bytes(s.N) + lib().gdr_sim_topk_prefilter_workspace_bytes(s.B, s.N, s.d, s.k)
    ws = torch.empty(need, dtype=torch.uint8, device=s.Qd.device)
    _fill(ws, s.B, s.N, live, allowed)
    v, i, st = _out(s.B, s.k, s.Qd.device)
    rc = lib().gdr_sim_topk_prefilter_masked(ptr(s.Qd), s.B, ptr(s.Dd), ptr(s.P.D16), s.P.dnorm_max, s.N, s.d, s.k, idx_offset, ptr(v),
                                             ptr(i), ptr(st), flags, ptr(ws), need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return v, i, st


def _compacted(s, rows_allowed, qs, k):
    """gdr_sim_topk_prefilter over D[allowed], D16[allowed] with the same dnorm_max for the queries qs; ids mapped back."""
    rows = np.nonzero(rows_allowed)[0]
    sel = torch.from_numpy(rows).to(s.Dd.device)
    cv, ci, cst = _plain(s.Qd[qs].contiguous(), s.Dd[sel].contiguous(), s.P.D16[sel].contiguous(), s.P.dnorm_max, k)
    assert int(cst.abs().sum()) == 0, "the compacted call flagged: it is no oracle for this case"
    return cv, rows[ci.cpu().numpy().astype(np.int64)]


def _check(s, allowed, v, i, what):
    """The three oracles for a result whose status is 0 everywhere.  allowed: bool [N] (every query) or bool [B, N]."""
    vv, iv = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    per_query = allowed.ndim == 2
    groups = [(slice(q, q + 1), allowed[q]) for q in range(s.B)] if per_query else [(slice(0, s.B), allowed)]
    for qs, a in groups:
        c = int(min(a.sum(), s.k))
        assert (iv[qs, c:] == -1).all() and np.isneginf(vv[qs, c:]).all(), f"{what}: the tail of a short list is -inf / -1"
        if c == 0:
            continue
        assert (iv[qs, :c] >= 0).all() and a[iv[qs, :c]].all(), f"{what}: a disallowed row was returned"
        rv, ri = live_ref.topk(s.S[qs], a, c)
        order_insensitive_topk_match(rv, ri, vv[qs, :c], iv[qs, :c], TOL)
        cv, ci = _compacted(s, a, qs, c)
        assert np.array_equal(iv[qs, :c], ci), f"{what}: ids differ from gdr_sim_topk_prefilter over the allowed rows"
        assert torch.equal(v[qs, :c], cv), f"{what}: values are not the bits of gdr_sim_topk_prefilter over the allowed rows"


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_live_mask_through_the_prefilter(dev, shape, mask):
    s = _data(shape, dev)
    assert s.stride == STRIDE.get(shape, 39)
    top = np.union1d(np.unique(s.i0.cpu().numpy()), np.unique(s.ref_top[:, :s.k]))
    live = live_mask(s, mask, top=top)
    assert int(live.sum()) >= s.k
    longest, fullest = assert_cannot_flag(s, np.broadcast_to(live, (s.B, s.N)), f"{shape} / {mask}")
    print(f"{shape} / {mask}: list {longest}, band {fullest}")
    v, i, st = _masked(s, live=live)
    assert int(st.abs().sum()) == 0
    if mask == "none":
        assert torch.equal(v, s.v0) and torch.equal(i, s.i0), "nothing dead: not gdr_sim_topk_prefilter's result bit for bit"
    if mask == "topk_union":
        assert not np.isin(i.cpu().numpy(), s.i0.cpu().numpy()).any()
    _check(s, live, v, i, f"{shape} / {mask}")
    v2, i2, st2 = _masked(s, live=live, idx_offset=1000)
    assert torch.equal(v2, v) and torch.equal(i2, i + 1000) and int(st2.abs().sum()) == 0


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_query_masks_through_the_prefilter(dev, shape, mask):
    s = _data(shape, dev)
    i0 = s.i0.cpu().numpy()
    a = query_masks(s, mask, top=[np.union1d(i0[q], s.ref_top[q, :s.k]) for q in range(s.B)])
    assert a[0].all() and len({a[q].tobytes() for q in range(s.B)}) >= min(s.B, 3)
    longest, fullest = assert_cannot_flag(s, a, f"{shape} / per-query {mask}")
    print(f"{shape} / per-query {mask}: list {longest}, band {fullest}")
    v, i, st = _masked(s, allowed=a)
    assert int(st.abs().sum()) == 0
    assert torch.equal(v[0], s.v0[0]) and torch.equal(i[0], s.i0[0]), "query 0 allows everything: gdr_sim_topk_prefilter's row bit for bit"
    assert not np.isin(i[1].cpu().numpy(), s.ref_top[1, :200]).any()
    if mask == "topk_union" and shape != "stride1_B4":
        for q in range(2, s.B):
            assert not np.isin(i[q].cpu().numpy(), i0[q]).any()
    if shape == "stride1_B4":
        assert (i[2] == -1).all() and torch.isneginf(v[2]).all(), "the empty bitmap"
        assert (i[3, 7:] == -1).all() and torch.isneginf(v[3, 7:]).all() and (i[3, :7] >= 0).all()
    _check(s, a, v, i, f"{shape} / per-query {mask}")
    v2, i2, _ = _masked(s, allowed=a, idx_offset=1000)
    assert torch.equal(v2, v) and torch.equal(i2, torch.where(i >= 0, i + 1000, i))


@pytest.mark.parametrize("shape", ["sampled_B4", "sampled_B40", "stream_B4"])
def test_fewer_than_k_allowed_sample_rows(dev, shape):
    """Every row of every sample tile dead except 5 (k = 10): the sample gives no threshold, the fix-up lowers it to -inf, the filter pass
    keeps all other rows and the list overflows — status 1 for every query; a list with status 0 must be the restatement's.
    ops.sim_topk over PrefilteredCorpus(masks=True) repairs the flagged queries (exhaustive fp32 with the mask) and is exact."""
    s = _data(shape, dev)
    assert s.stride == 39 and s.k == 10
    inside = in_sample_tile(s.N, s.stride)
    live = ~inside
    live[np.argsort(-np.where(inside, s.S[0], -np.inf))[:5]] = True
    assert int((live & inside).sum()) == 5
    assert occupancy(s.S16, np.broadcast_to(live, (s.B, s.N)), s.Q, s.dnorm, s.d, s.k)[4] == list(range(s.B))
    rv, ri = live_ref.topk(s.S, live, s.k)
    for kw in ({"live": live}, {"allowed": np.broadcast_to(live, (s.B, s.N))}):
        v, i, st = _masked(s, **kw)
        st = st.cpu().numpy()
        assert (st == 1).all(), "the sample gave no threshold: every query must be flagged"
        ok = st == 0
        order_insensitive_topk_match(rv[ok], ri[ok], v.cpu().numpy()[ok], i.cpu().numpy().astype(np.int64)[ok], TOL)
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    ov, oi, ost = ops.sim_topk(s.Qd, ops.PrefilteredCorpus(s.Dd, masks=True), s.k, live=L, return_status=True)
    assert int(ost.abs().sum()) == 0 and live[oi.cpu().numpy().astype(np.int64)].all()
    order_insensitive_topk_match(rv, ri, ov.cpu().numpy(), oi.cpu().numpy().astype(np.int64), TOL)
    # a query of its own with a short sample loses its own threshold only
    a = np.ones((s.B, s.N), bool)
    a[2] = live
    v, i, st = _masked(s, allowed=a)
    assert st.cpu().tolist() == [1 if q == 2 else 0 for q in range(s.B)]
    keep = [q for q in range(s.B) if q != 2]
    assert torch.equal(v[keep], s.v0[keep]) and torch.equal(i[keep], s.i0[keep])


@pytest.mark.parametrize("flag", [LIVE, QM])
@pytest.mark.parametrize("shape", ["ragged_B4", "sampled_B40", "stream_B4", "stride1_B4"])
def test_memory_contract(dev, shape, flag):
    """A workspace of exactly the declared size between guard bands: the scratch behind the bitmaps poisoned, the bitmap region
    (garbage in the ignored bits past N and in the padding) byte-identical after the call, guarded outputs, operands with winning
    rows behind them, a non-default stream.  One byte less: GDR_ENOSPC and nothing launched; every refused flag: GDR_EINVAL likewise."""
    s = _data(shape, dev)
    if flag == LIVE:
        allowed = live_mask(s, "topk_union") & (np.random.default_rng(5).random(s.N) < 0.9)
        maps = allowed[None]
    else:
        allowed = maps = query_masks(s, "outside_sample_tiles")
    assert_cannot_flag(s, np.broadcast_to(allowed, (s.B, s.N)), f"{shape} / memory contract")
    M, W = mask_bytes(s.N), (s.N + 31) // 32
    need = lib().gdr_sim_topk_prefilter_masked_workspace_bytes(s.B, s.N, s.d, s.k, flag)
    region = np.full((maps.shape[0], M), 0xA7, np.uint8)
    for q, a in enumerate(maps):
        words = live_ref.pack(a).copy()
        if s.N % 32:
            words[-1] |= np.int32(-1) << np.int32(s.N % 32)                  # bits past N: ignored
        region[q, :W * 4] = words.view(np.uint8)
    region = torch.from_numpy(region.reshape(-1)).to(dev)
    Qd, qh = guarded_input(s.Qt, tail=torch.full((128, s.d), 1e3))
    Dd, dh = guarded_input(s.Dt, tail=torch.full((256, s.d), 10.0))          # rows that would win every top-k if read
    D16, d16h = guarded_input(s.Dt.bfloat16(), tail=torch.full((256, s.d), 10.0, dtype=torch.bfloat16))
    fn = lib().gdr_sim_topk_prefilter_masked
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill in (0x00, 0xFF, 0x5A):
        ws, hws = poisoned_workspace(need, fill, dev)
        ws[:region.numel()].copy_(region)
        v, hv = guarded((s.B, s.k), torch.float32, dev)
        i, hi = guarded((s.B, s.k), torch.int32, dev)
        st, hst = guarded((s.B,), torch.int32, dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        for rep in range(2 if fill == 0x5A else 1):                           # the last fill runs twice on the warm workspace
            with torch.cuda.stream(side):
                assert stream_ptr().value == side.cuda_stream and side.cuda_stream != 0
                rc = fn(ptr(Qd), s.B, ptr(Dd), ptr(D16), s.P.dnorm_max, s.N, s.d, s.k, 0, ptr(v), ptr(i), ptr(st), flag, ptr(ws), need,
                        stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            side.synchronize()
            tag = f"{shape} fill 0x{fill:02X} run {rep}"
            for h, name in ((hws, "workspace"), (hv, "out_val"), (hi, "out_idx"), (hst, "status")):
                h.check(f"{tag}: {name}")
            assert torch.equal(ws[:region.numel()], region), f"{tag}: the bitmap region was written"
            runs.append((v.clone(), i.clone(), st.clone()))
    n0 = lib().gdr_launch_count()
    assert fn(ptr(Qd), s.B, ptr(Dd), ptr(D16), s.P.dnorm_max, s.N, s.d, s.k, 0, ptr(v), ptr(i), ptr(st), flag, ptr(ws), need - 1,
              stream_ptr()) == _ffi.GDR_ENOSPC
    assert str(need).encode() in lib().gdr_last_error() and lib().gdr_launch_count() == n0
    for bad in REFUSED_FLAGS:
        assert fn(ptr(Qd), s.B, ptr(Dd), ptr(D16), s.P.dnorm_max, s.N, s.d, s.k, 0, ptr(v), ptr(i), ptr(st), bad, ptr(ws), need,
                  stream_ptr()) == _ffi.GDR_EINVAL, bad
        assert lib().gdr_launch_count() == n0, bad
    hws.check("workspace after the refused calls")
    assert torch.equal(v, runs[-1][0]) and torch.equal(i, runs[-1][1]), "a refused call wrote its outputs"
    for h, name in ((qh, "Q"), (dh, "D"), (d16h, "D_bf16")):
        h.unchanged(name)
    assert lib().gdr_device_fault_pending() == 0
    for v, i, st in runs:
        assert int(st.abs().sum()) == 0
        assert torch.equal(v, runs[0][0]) and torch.equal(i, runs[0][1]), "the result depends on what the scratch held"
    _check(s, allowed, runs[0][0], runs[0][1], shape)


@pytest.mark.parametrize("shape", ["sampled_B40", "stream_B4", "k100_B40"])
def test_two_runs_are_bit_identical(dev, shape):
    s = _data(shape, dev)
    live, a = live_mask(s, "outside_sample_tiles"), query_masks(s, "none")
    for kw in ({"live": live}, {"allowed": a}):
        x, y = _masked(s, **kw), _masked(s, **kw)
        assert all(torch.equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("flag", [LIVE, QM])
@pytest.mark.parametrize("shape", ["sampled_B40", "stream_B4"])
def test_masked_call_in_a_captured_graph(dev, shape, flag):
    """The C call captured in a graph and replayed; then the bitmap(s) in the workspace are rewritten and the replay follows them."""
    s = _data(shape, dev)
    first = live_mask(s, "topk_union") if flag == LIVE else query_masks(s, "topk_union")
    second = first & live_mask(s, "outside_sample_tiles") if flag == LIVE else query_masks(s, "inside_sample_tiles")
    for m in (first, second):
        assert_cannot_flag(s, np.broadcast_to(m, (s.B, s.N)), f"{shape} / graph")
    kw = (lambda m: {"live": m}) if flag == LIVE else (lambda m: {"allowed": m})
    need = lib().gdr_sim_topk_prefilter_masked_workspace_bytes(s.B, s.N, s.d, s.k, flag)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gv, gi, gst = _out(s.B, s.k, dev)

    def call():
        rc = lib().gdr_sim_topk_prefilter_masked(ptr(s.Qd), s.B, ptr(s.Dd), ptr(s.P.D16), s.P.dnorm_max, s.N, s.d, s.k, 0, ptr(gv), ptr(gi),
                                                 ptr(gst), flag, ptr(ws), need, stream_ptr())
        assert rc == 0, lib().gdr_last_error().decode()

    _fill(ws, s.B, s.N, **kw(first))
    warm = torch.cuda.Stream(device=dev)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        call()                                                                # eager; also the one run a capture needs first
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for m in (first, first, second):
        _fill(ws, s.B, s.N, **kw(m))
        gv.zero_(), gi.zero_(), gst.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        ev, ei, est = _masked(s, **kw(m))
        assert torch.equal(gv, ev) and torch.equal(gi, ei) and torch.equal(gst, est) and int(gst.abs().sum()) == 0
    _check(s, second, gv, gi, f"{shape}: graph replay after the bitmap changed")


# ----------------------------------------------------------------------------------------------------------- ops.sim_topk routing
def test_routing_default_object_keeps_the_plain_path_and_masks_true_takes_the_prefilter(dev, monkeypatch):
    s = _data("sampled_B40", dev)
    live = live_mask(s, "topk_union")
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    ov, oi = ops.sim_topk(s.Qd, s.Dd, s.k, live=L)
    pv, pi = ops.sim_topk(s.Qd, ops.PrefilteredCorpus(s.Dd), s.k, live=L)
    assert torch.equal(pv, ov) and torch.equal(pi, oi), "the default object must stay on the plain fp32 path bit for bit"
    PM = ops.PrefilteredCorpus(s.Dd, masks=True)
    seen = []
    real = ops._sim_topk_prefilter_raw
    monkeypatch.setattr(ops, "_sim_topk_prefilter_raw", lambda *a, **k: seen.append(a) or real(*a, **k))
    mv, mi, mst = ops.sim_topk(s.Qd, PM, s.k, live=L, return_status=True)
    assert len(seen) == 1 and int(mst.abs().sum()) == 0
    rv, ri, rst = _masked(s, live=live)
    assert torch.equal(mv, rv) and torch.equal(mi, ri), "masks=True: the masked pre-filter's bits"
    assert torch.equal(mi, oi), "the same documents as the plain call"
    order_insensitive_topk_match(ov.cpu().numpy(), oi.cpu().numpy(), mv.cpu().numpy(), mi.cpu().numpy(), TOL)
    # live= and allowed= together are their AND
    a = query_masks(s, "none")
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    bv, bi = ops.sim_topk(s.Qd, PM, s.k, live=L, allowed=R)
    assert np.array_equal(R.to_bool().cpu().numpy(), a), "sim_topk must not change the caller's QueryRows"
    rv, ri, rst = _masked(s, allowed=a & live)
    assert int(rst.abs().sum()) == 0 and torch.equal(bv, rv) and torch.equal(bi, ri)
    # outside the pre-filter's conditions the masked call is the plain one, launch for launch
    n = len(seen)
    ev, ei = ops.sim_topk(s.Qd, PM, s.k, live=L, flags=_ffi.SIM_EXHAUSTIVE)
    xv, xi = ops.sim_topk(s.Qd, s.Dd, s.k, live=L, flags=_ffi.SIM_EXHAUSTIVE)
    assert len(seen) == n and torch.equal(ev, xv) and torch.equal(ei, xi)


def test_routing_gather_auto_sends_only_the_wide_remainder_to_the_masked_prefilter(dev, monkeypatch):
    s = _data("sampled_B4", dev)
    monkeypatch.setattr(ops, "GATHER_MAX_ROWS", 8192)                         # the routing bound, scaled down to this corpus of 20 000 rows
    a = query_masks(s, "none")                                                # all rows, all but 200, a narrow one below, a random half
    a[2] = False
    a[2, np.random.default_rng(3).choice(s.N, 3000, replace=False)] = True    # narrow: the gather mode's
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    PM = ops.PrefilteredCorpus(s.Dd, masks=True)
    assert (a.sum(1) <= ops.GATHER_MAX_ROWS).tolist() == [False, False, True, False]
    v, i, st = ops.sim_topk(s.Qd, PM, s.k, allowed=R, gather="auto", return_status=True)
    assert int(st.abs().sum()) == 0
    narrow, wide = [2], [0, 1, 3]
    gv, gi = ops.sim_topk(s.Qd[narrow].contiguous(), s.Dd, s.k, allowed=R.rows(narrow), gather="auto")
    assert torch.equal(v[narrow], gv) and torch.equal(i[narrow], gi), "narrow rows: the gather call's bits"
    w = types.SimpleNamespace(**vars(s))
    w.B, w.Qd = len(wide), s.Qd[wide].contiguous()
    wv, wi, wst = _masked(w, allowed=a[wide])
    assert int(wst.abs().sum()) == 0 and torch.equal(v[wide], wv) and torch.equal(i[wide], wi), "wide rows: the masked pre-filter's bits"
    vv, iv = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    for q in range(s.B):
        rv, ri = live_ref.topk(s.S[q:q + 1], a[q], s.k)
        order_insensitive_topk_match(rv, ri, vv[q:q + 1], iv[q:q + 1], TOL)


# ------------------------------------------------------------------------------------------------------------------ image upkeep
def test_update_rows_keeps_the_image_and_the_norm_bound(dev):
    N, d = 5_003, 64
    D = torch.from_numpy(synth.make_corpus(N, d, seed=9)).to(dev)
    P = ops.PrefilteredCorpus(D.clone(), masks=True)
    rng = np.random.default_rng(2)
    ids = np.concatenate([[0, N - 1, 17, 17], rng.choice(N, 300, replace=False)])
    new = torch.from_numpy(rng.standard_normal((ids.size, d)).astype(np.float32) * 0.05).to(dev)
    P.D[torch.from_numpy(ids).to(dev)] = new                                  # (the repeated id: the last write wins, whichever it is)
    before = P.dnorm_max
    n0 = lib().gdr_launch_count()
    P.update_rows(ids)
    assert lib().gdr_launch_count() == n0 + 1
    assert torch.equal(P.D16.view(torch.int16), ops.to_bf16(P.D).view(torch.int16)), "the image is not gdr_cast_f32_bf16's bits"
    true_max = float(torch.linalg.vector_norm(P.D.double(), dim=1).max())
    assert P.dnorm_max >= before and P.dnorm_max >= true_max * (1 - 1e-6)     # smaller rows came in: the bound only grows
    big = int(ids[5])
    P.D[big] *= 40.0
    P.update_rows(torch.tensor([big], device=dev))
    grown = P.dnorm_max
    assert torch.equal(P.D16.view(torch.int16), ops.to_bf16(P.D).view(torch.int16))
    assert grown == P.refresh().dnorm_max, "the largest row was among the ids: a full refresh gives the same bound, bit for bit"
    with pytest.raises(_ffi.GdrError, match="row ids must lie"):
        P.update_rows([N])
    with pytest.raises(_ffi.GdrError, match="row ids must lie"):
        P.update_rows(torch.tensor([-1], device=dev))
    assert P.update_rows([]) is P
    # the C call: n_rows = 0 launches nothing, d % 8 != 0 is refused
    n0 = lib().gdr_launch_count()
    m = torch.zeros(1, device=dev)
    assert lib().gdr_prefilter_update_rows(ptr(P.D), ptr(P.D16), d, None, 0, ptr(m), stream_ptr()) == 0
    assert lib().gdr_prefilter_update_rows(ptr(P.D), ptr(P.D16), 12, ptr(m), 1, ptr(m), stream_ptr()) == _ffi.GDR_EINVAL
    assert lib().gdr_launch_count() == n0


def test_update_rows_memory_contract(dev):
    """Only the listed rows of the image change; D, the ids and the bands around everything stay as they were."""
    N, d = 1_001, 72                                                          # d % 8 == 0, not a multiple of the 256-column step
    Dh = torch.from_numpy(synth.make_corpus(N, d, seed=4))
    ids = torch.tensor([0, N - 1, 5, 5, 640, 333], dtype=torch.int32)
    Dd, dh = guarded_input(Dh, tail=torch.full((256, d), 7.0))
    rows, rh = guarded_input(ids, tail=torch.full((1024,), N + 5, dtype=torch.int32))
    D16, h16 = guarded((N, d), torch.bfloat16, dev)
    D16.fill_(3.0)
    m, hm = guarded((1,), torch.float32, dev)
    m.fill_(0.25)
    assert lib().gdr_prefilter_update_rows(ptr(Dd), ptr(D16), d, ptr(rows), ids.numel(), ptr(m), stream_ptr()) == 0, lib().gdr_last_error()
    for h, name in ((h16, "D_bf16"), (hm, "norm2_max")):
        h.check(name)
    dh.unchanged("D")
    rh.unchanged("rows")
    want = torch.full((N, d), 3.0, dtype=torch.bfloat16)
    want[ids.long()] = Dh.bfloat16()[ids.long()]
    assert torch.equal(D16.cpu().view(torch.int16), want.view(torch.int16))
    n2 = torch.empty(1, device=dev)
    sub = Dh[ids.long()].to(dev).contiguous()
    assert lib().gdr_row_norm2_max(ptr(sub), sub.shape[0], d, ptr(n2), stream_ptr()) == 0
    assert float(n2) > 0.25 and float(m) == float(n2), "not raised to gdr_row_norm2_max of the listed rows"
    m.fill_(100.0)
    assert lib().gdr_prefilter_update_rows(ptr(Dd), ptr(D16), d, ptr(rows), ids.numel(), ptr(m), stream_ptr()) == 0
    assert float(m) == 100.0, "the bound was lowered"


def test_rebind_keeps_the_old_image_and_covers_the_new_rows(dev):
    N, d, n = 3_000, 64, 2_000
    Dall = torch.from_numpy(synth.make_corpus(N + n, d, seed=6)).to(dev)
    P = ops.PrefilteredCorpus(Dall[:N].clone(), masks=True)
    old_buf = P.D16.data_ptr()
    P.D16[7].fill_(123.0)                                                     # a mark: the old rows' image is kept, not re-derived
    grown = torch.empty((N + n, d), dtype=torch.float32, device=dev)          # a reallocated corpus buffer
    grown.copy_(Dall)
    P.rebind(grown)
    assert P.D.data_ptr() == grown.data_ptr() and P.shape == (N + n, d) and P.D16.shape == (N + n, d) and P.D16.data_ptr() != old_buf
    want = ops.to_bf16(grown)
    assert bool((P.D16[7] == 123.0).all())
    P.update_rows([7])
    assert torch.equal(P.D16.view(torch.int16), want.view(torch.int16))
    assert P.dnorm_max >= float(torch.linalg.vector_norm(grown.double(), dim=1).max()) * (1 - 1e-6)
    cap = P._D16_buf.shape[0]
    assert cap >= N + N // 2 and P.rebind(grown[:N + n]).D16.data_ptr() == P._D16_buf.data_ptr() and P._D16_buf.shape[0] == cap
    with pytest.raises(_ffi.GdrError, match="rebind"):
        P.rebind(grown[:N])
    # a search over the grown corpus, masked: exact
    Q = torch.from_numpy(synth.make_queries(Dall.cpu().numpy(), 4, seed=1)[0]).to(dev)
    live = np.ones(N + n, bool)
    live[::3] = False
    v, i = ops.sim_topk(Q, P, 10, live=ops.LiveRows.from_bool(torch.from_numpy(live).to(dev)))
    rv, ri = live_ref.topk(live_ref.scores(Q.cpu().numpy(), Dall.cpu().numpy()), live, 10)
    order_insensitive_topk_match(rv, ri, v.cpu().numpy(), i.cpu().numpy().astype(np.int64), TOL)


# ------------------------------------------------------------------------------------------------------------------ the retriever
def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=4, length_penalty=0.8, kary=V,
                                 position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_retriever_search_prefilter_follows_the_document_lifecycle(dev, monkeypatch):
    """add -> remove -> update -> restore with search_prefilter=True: after each step search() matches the restatement over the live
    rows with the current embeddings, goes through the masked pre-filter, and the image equals doc_embed.bfloat16() on every live row."""
    from gdr_amd.modeling import GDRRetriever
    V, csz, d, k, B = 30, 3, 64, 20, 6
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N0 = len(names) * csz
    D0 = synth.make_corpus(N0, d, cluster_size=csz, seed=8)
    Q, _ = synth.make_queries(D0, B, seed=3)
    Qd = torch.from_numpy(Q).to(dev)
    mk = lambda: codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N0, dtype=np.int32))   # noqa: E731
    r = GDRRetriever(None, torch.from_numpy(D0).to(dev), mk(), _args(V), search_prefilter=True)
    plain = GDRRetriever(None, torch.from_numpy(D0).to(dev), mk(), _args(V))
    calls = []
    real = ops._sim_topk_prefilter_raw
    monkeypatch.setattr(ops, "_sim_topk_prefilter_raw", lambda *a, **kw: calls.append(a) or real(*a, **kw))

    def step(what):
        N = r.doc_embed.shape[0]
        live = np.zeros(N, bool)
        live[np.asarray(r.index.members)] = True
        n = len(calls)
        v, i = r.search(Qd, k)
        assert len(calls) == n + 1 and calls[-1][5] is r.live_rows, f"{what}: not served by the masked pre-filter"
        assert i.dtype == torch.int64 and live[i.cpu().numpy()].all()
        rv, ri = live_ref.topk(live_ref.scores(Q, r.doc_embed.cpu().numpy()), live, k)
        order_insensitive_topk_match(rv, ri, v.cpu().numpy(), i.cpu().numpy(), TOL)
        P = r._prefiltered
        assert P.D.data_ptr() == r.doc_embed.data_ptr() and P.shape == r.doc_embed.shape
        rows = torch.from_numpy(np.nonzero(live)[0]).to(dev)
        assert torch.equal(P.D16[rows].view(torch.int16), r.doc_embed[rows].bfloat16().view(torch.int16)), f"{what}: stale image"
        assert P.dnorm_max >= float(torch.linalg.vector_norm(r.doc_embed[rows].double(), dim=1).max()) * (1 - 1e-6)
        pv, pi = plain.search(Qd, k)                                          # the default retriever, taken through the same steps
        assert len(calls) == n + 1 and torch.equal(pi, i), f"{what}: other documents than the default retriever's"
        dv, di = ops.sim_topk(Qd, plain.doc_embed, k, live=plain.live_rows)
        assert torch.equal(pv, dv) and torch.equal(pi, di.to(torch.int64)), "the default retriever's search changed"
        return i.cpu().numpy()

    base = step("as built")
    X = (D0[base[:, 0]] * np.float32(1.01)).astype(np.float32)                # every query's best document again, a little longer
    for x in (r, plain):
        new_ids, _ = x.add_documents(torch.from_numpy(X).to(dev))
    got = step("add")
    assert r.doc_embed.shape[0] == N0 + B and np.isin(got, new_ids).any()
    gone = np.unique(np.concatenate([base[:, :5].reshape(-1), np.arange(0, N0, 7), np.arange(N0 - 40, N0)]))
    for x in (r, plain):
        x.remove_documents(gone)
    got = step("remove")
    assert not np.isin(got, gone).any(), "a removed document came back"
    moved = np.setdiff1d(np.arange(3, N0, 11), gone)[:200]
    E = np.random.default_rng(12).standard_normal((moved.size, d)).astype(np.float32) * np.float32(0.2)
    E[:B] = Q * np.float32(1.5)                                               # rewritten rows that must now win, longer than any row before
    for x in (r, plain):
        x.update_documents(moved, torch.from_numpy(E).to(dev))
    got = step("update")
    assert np.isin(got[:, 0], moved[:B]).all(), "the rewritten rows were searched through a stale image"
    back = gone[::3]
    for x in (r, plain):
        x.update_documents(back, torch.from_numpy(D0[back]).to(dev))          # restored, with their old embeddings
    got = step("restore")
    assert np.isin(got, back).any() and not np.isin(got, np.setdiff1d(gone, back)).any()
    with pytest.raises(_ffi.GdrError, match="sharded"):
        GDRRetriever(None, r.doc_embed, r.index, _args(V), sharded=types.SimpleNamespace(D=r.doc_embed), search_prefilter=True)
    with pytest.raises(_ffi.GdrError, match="fp32 doc_embed"):
        GDRRetriever(None, r.doc_embed.bfloat16(), r.index, _args(V), search_prefilter=True)
