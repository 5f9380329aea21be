"""Corpus search with a row filter per query on the MI355X: gdr_sim_topk / gdr_sim_topk_bf16 with
GDR_SIM_QUERY_MASK in every form sim_topk_impl has, against two oracles —
  (1) bit for bit: row q of the flagged call is row q of the GDR_SIM_LIVE_MASK call (same Q, B, D, other flags) given bitmap q as
      its one bitmap — both run the same plan and the same kernel forms, so this holds in every form, the split-K stream sample
      pass included.  A list that overflowed (status 1) holds whichever survivors won their slots and is compared by status only;
  (2) the numpy restatement (tests/live_ref.py) applied per query to what ops.sim_topk returns (exact for every query: it re-runs
      an overflowed one), under oracle/parity_rules.py's rule with the tolerance tests/test_gpu_live_search.py uses.  No case is
      skipped.  In the forms of 4 queries at k = 10 the reference's own gap between its k-th and (k + 1)-th allowed score is
      asserted to exceed the rule's tie width, 2 TOL (1 + |score|) ~ 4.5e-4, for every query and mask, so the id comparison is
      total there (the seeds were chosen on the CPU for that: QSEED).  One query in twenty has a closer pair at the cut, so no
      seed gives 40 queries x 6 masks without one, and at k = 1100 of 40 000 rows neighbouring scores are ~1e-5 apart for any
      seed: there the rule's own treatment of the last tie group applies (values within the tolerance, ids counted) —
then the memory contract of the mode (tests/abi_guard.py), determinism, graph capture, live= with allowed=, and
GDRRetriever.search(allowed=) after remove_documents."""
import types

import numpy as np
import pytest
import torch

import lifecycle_ref
import live_ref
import sim_widths
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import order_insensitive_topk_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

TOL = 1e-4                         # oracle/parity_rules.py: |got - ref| <= 1e-4 + 1e-4 |ref|, ids exact beyond twice that
LIVE, QM, EXH, NOSTREAM = _ffi.SIM_LIVE_MASK, 8, _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM

# form -> (B, N, d, k, flags, bf16).  The fp32 stream kernels serve B <= 32 at d % 128 == 0 (bf16: d % 256 == 0), their small sample
# pass is the split-K one; everything else is the tiled GEMM core.  A sampled plan needs N > 16 384.
FORMS = {
    "stream_B4": (4, 20_000, 128, 10, 0, False),                    # latency mode: stream kernels, sliced threshold / select tails
    "stream_ragged_B4": (4, 20_001, 128, 10, 0, False),             # a last tile of one row
    "no_stream_B4": (4, 20_000, 128, 10, NOSTREAM, False),          # the same shape forced onto the tiled core
    "tiled_ragged_B4": (4, 20_001, 64, 10, 0, False),
    "tiled_B40": (40, 20_000, 64, 10, 0, False),
    "tiled_ragged_B40": (40, 20_001, 128, 10, 0, False),
    "deep_select_B4": (4, 40_000, 64, 1100, 0, False),              # k > 1024: the deep form of launch_select
    "bf16_B40": (40, 20_000, 64, 10, 0, True),
    "bf16_stream_B4": (4, 20_001, 256, 10, 0, True),
    "exhaustive_B4": (4, 20_000, 64, 10, EXH, False),
    "stride1_B4": (4, 5000, 64, 10, 0, False),                      # sample pass and its mask only
}
QSEED = {"stream_ragged_B4": 1}                                     # the query seed where B + d leaves a reference tie at the cut
STRIDE = {"deep_select_B4": 6, "exhaustive_B4": 1, "stride1_B4": 1}  # every other form: 39
MASKS = ("all", "halves", "own_topk_denied", "seven_rows", "outside_sample_tiles", "two_percent")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


_HOST, _DATA = {}, {}


def _host(form):
    """Per form, made once and never modified, on the host: the operands, the fp64 scores of the operands as the kernel sees them.
    A few rows are exact copies of a query's best rows: exact ties inside the top-k."""
    if form not in _HOST:
        B, N, d, k, flags, bf16 = FORMS[form]
        D = synth.make_corpus(N, d, seed=N + d)
        Q, _ = synth.make_queries(D, B, seed=QSEED.get(form, B + d))
        for q in range(min(B, 2)):
            src = np.argsort(-(D @ Q[q]))[:2]
            D[(src + 777) % N] = D[src]
        Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
        if bf16:
            Qt, Dt = Qt.bfloat16(), Dt.bfloat16()
        S = live_ref.scores(Qt.double().numpy(), Dt.double().numpy())
        _HOST[form] = types.SimpleNamespace(form=form, B=B, N=N, d=d, k=k, flags=flags, bf16=bf16, S=S, Qt=Qt, Dt=Dt,
                                            stride=sim_widths.plan(N, k, bool(flags & EXH))[0])
    return _HOST[form]


def _data(form, dev):
    """_host(form) with the operands on the device and the unflagged result beside them."""
    if form not in _DATA:
        s = types.SimpleNamespace(**vars(_host(form)))
        s.Qd, s.Dd = s.Qt.to(dev), s.Dt.to(dev)
        s.v0, s.i0, st0 = _raw(s.Qd, s.Dd, s.k, s.flags)
        assert int(st0.abs().sum()) == 0
        _DATA[form] = s
    return _DATA[form]


def _raw(Qd, Dd, k, flags, live=None, allowed=None, idx_offset=0):
    """The C entry point with a workspace of exactly the declared size.  live: bool numpy [N] -> the GDR_SIM_LIVE_MASK call;
    allowed: bool numpy [B, N] -> the GDR_SIM_QUERY_MASK call, bitmap q at byte q * M."""
    B, d = Qd.shape
    N = Dd.shape[0]
    flags |= (LIVE if live is not None else 0) | (QM if allowed is not None else 0)
    need = lib().gdr_sim_topk_workspace_bytes(B, N, d, k, flags)
    ws = torch.empty(need, dtype=torch.uint8, device=Qd.device)
    if live is not None:
        words = torch.from_numpy(live_ref.pack(live)).to(Qd.device)
        ws[:words.numel() * 4].view(torch.int32).copy_(words)
    if allowed is not None:
        M, W = live_ref.mask_bytes(N), (N + 31) // 32
        words = torch.from_numpy(np.stack([live_ref.pack(a) for a in allowed])).to(Qd.device)
        ws[:B * M].view(torch.int32).view(B, M // 4)[:, :W].copy_(words)
    v = torch.empty((B, k), dtype=torch.float32, device=Qd.device)
    i = torch.empty((B, k), dtype=torch.int32, device=Qd.device)
    st = torch.empty((B,), dtype=torch.int32, device=Qd.device)
    fn = lib().gdr_sim_topk_bf16 if Qd.dtype == torch.bfloat16 else lib().gdr_sim_topk
    rc = fn(ptr(Qd), B, ptr(Dd), N, d, k, idx_offset, ptr(v), ptr(i), ptr(st), flags, ptr(ws), need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return v, i, st


def _allowed(s, name, top):
    """(bool [B, N], set of queries the raw call of a SAMPLED plan must flag): a different bitmap per query in every case.
    top: int [B, k], every query's unfiltered top-k."""
    rng = np.random.default_rng(len(name) + s.N + s.B)
    a = np.ones((s.B, s.N), bool)
    flagged = set()
    if name != "all":
        for q in range(s.B):
            a[q] = rng.random(s.N) < 0.5                                      # independent halves
    if name == "all":
        pass
    elif name == "own_topk_denied":
        a[:] = True
        for q in range(s.B):
            a[q, top[q]] = False
    elif name == "seven_rows":                                                # query 0 unrestricted beside query 1 with 7 rows
        a[0] = True
        a[1] = False
        a[1, [0, 31, 32, 4000, 4777, s.N - 2, s.N - 1]] = True
        flagged = {1}                                                         # 7 < k allowed sample rows: thr = -inf, the list overflows
    elif name == "outside_sample_tiles":                                      # query 2 allows no row of a sample tile
        a[2] = ~sim_widths.in_sample_tile(s.N, s.stride) if s.stride > 1 else rng.random(s.N) < 0.5
        flagged = {2}
    elif name == "two_percent":                                               # query 3 allows 2 % beside unrestricted ones
        a[:] = True
        a[3] = rng.random(s.N) < 0.02
        flagged = {3}
    return a, (flagged if s.stride > 1 else set())


def _reference(s, a):
    """live_ref's restatement per query: (values fp64 [B, k], ids int64 [B, k], allowed counts [B])."""
    rv, ri = np.empty((s.B, s.k)), np.empty((s.B, s.k), np.int64)
    for q in range(s.B):
        rv[q], ri[q] = (x[0] for x in live_ref.topk(s.S[q:q + 1], a[q], s.k))
    return rv, ri, a.sum(1)


def _gap_ok(s, a):
    """The reference's k-th and (k + 1)-th allowed scores are further apart than the parity rule's tie width, for every query."""
    for q in range(s.B):
        v = np.sort(s.S[q, a[q]])[::-1]
        if v.size > s.k and not v[s.k - 1] - v[s.k] > 2 * TOL * (1 + abs(v[s.k - 1])):
            return False
    return True


def _check_exact(s, a, v, i, what):
    """Oracle 2 for a result that claims to be exact for every query (device tensors v, i without idx_offset)."""
    vv, iv = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    rv, ri, cnt = _reference(s, a)
    if s.k == 10 and s.B == 4:
        assert _gap_ok(s, a), f"{what}: the reference has a tie at the cut; choose another seed"
    for q in range(s.B):
        c = int(min(cnt[q], s.k))
        assert (iv[q, c:] == -1).all() and np.isneginf(vv[q, c:]).all(), f"{what}: query {q}: the tail of a short list is -inf / -1"
        assert (iv[q, :c] >= 0).all() and a[q, iv[q, :c]].all(), f"{what}: query {q} was given a row its bitmap denies"
        order_insensitive_topk_match(rv[q:q + 1, :c], ri[q:q + 1, :c], vv[q:q + 1, :c], iv[q:q + 1, :c], TOL)


def _check_raw(s, a, flagged, v, i, st, what):
    """Oracle 1 and the status contract of one raw flagged call."""
    stn = st.cpu().numpy()
    assert set(np.nonzero(stn)[0].tolist()) == flagged and set(stn.tolist()) <= {0, 1}, f"{what}: status {stn.tolist()}, expected 1 for {sorted(flagged)} only"
    for q in range(s.B):
        lv, li, lst = _raw(s.Qd, s.Dd, s.k, s.flags, live=a[q])
        assert int(lst[q]) == int(stn[q]), f"{what}: query {q}: status differs from the GDR_SIM_LIVE_MASK call given its bitmap"
        if stn[q] == 0:
            assert torch.equal(i[q], li[q]), f"{what}: query {q}: ids differ from the GDR_SIM_LIVE_MASK call given its bitmap"
            assert torch.equal(v[q], lv[q]), f"{what}: query {q}: values are not the bits of the GDR_SIM_LIVE_MASK call given its bitmap"


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("form", list(FORMS))
def test_filtered_topk_in_every_form(dev, form, mask):
    s = _data(form, dev)
    assert s.stride == STRIDE.get(form, 39)
    a, flagged = _allowed(s, mask, s.i0.cpu().numpy())
    v, i, st = _raw(s.Qd, s.Dd, s.k, s.flags, allowed=a)
    _check_raw(s, a, flagged, v, i, st, f"{form} / {mask}")
    if mask == "all":
        assert torch.equal(v, s.v0) and torch.equal(i, s.i0), "everything allowed: not the unflagged result bit for bit"
    if mask == "own_topk_denied":
        # fails without the feature (bit 8 of flags was ignored): every query is denied exactly the rows it used to get
        iv, i0 = i.cpu().numpy(), s.i0.cpu().numpy()
        assert not any(np.isin(iv[q], i0[q]).any() for q in range(s.B))
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    ov, oi, ost = ops.sim_topk(s.Qd, s.Dd, s.k, flags=s.flags, allowed=R, return_status=True)
    assert int(ost.abs().sum()) == 0
    ok = torch.from_numpy(st.cpu().numpy() == 0).to(dev)
    assert torch.equal(ov[ok], v[ok]) and torch.equal(oi[ok], i[ok]), "ops.sim_topk changed a list that was not flagged"
    _check_exact(s, a, ov, oi, f"{form} / {mask}")
    if mask == "seven_rows":
        assert (oi[1, 7:] == -1).all() and torch.isneginf(ov[1, 7:]).all() and (oi[1, :7] >= 0).all() and (oi[0] >= 0).all()
    if mask == "halves":                                                      # ids are row + idx_offset
        v2, i2, _ = _raw(s.Qd, s.Dd, s.k, s.flags, allowed=a, idx_offset=1000)
        assert torch.equal(v2, v) and torch.equal(i2, i + 1000)


@pytest.mark.parametrize("form", ["stream_B4", "tiled_B40", "bf16_B40", "stride1_B4"])
def test_equal_bitmaps_are_the_live_mask_call(dev, form):
    s = _data(form, dev)
    live = np.random.default_rng(11).random(s.N) < 0.5
    live[np.unique(s.i0.cpu().numpy())] = False
    a = np.broadcast_to(live, (s.B, s.N))
    got, want = _raw(s.Qd, s.Dd, s.k, s.flags, allowed=a), _raw(s.Qd, s.Dd, s.k, s.flags, live=live)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and int(got[2].abs().sum()) == 0


@pytest.mark.parametrize("form", ["stream_ragged_B4", "tiled_ragged_B40", "stride1_B4"])
def test_memory_contract_of_the_mode(dev, form):
    """A workspace of exactly gdr_sim_topk_workspace_bytes(.., flags | QUERY_MASK) between guard bands: the scratch behind the
    bitmaps poisoned, the B * M bitmap region (garbage in the ignored bits past N and in every bitmap's padding up to M)
    bit-identical after the call, guarded outputs, operands with winning rows behind them, a non-default stream, two runs."""
    s = _data(form, dev)
    a, _ = _allowed(s, "halves", None)
    i0 = s.i0.cpu().numpy()
    for q in range(s.B):
        a[q, i0[q]] = False
    M, W = live_ref.mask_bytes(s.N), (s.N + 31) // 32
    flags = s.flags | QM
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, flags)
    assert need == lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, s.flags) + s.B * M
    words = np.stack([live_ref.pack(r) for r in a])
    if s.N % 32:
        words[:, -1] |= np.int32(-1) << np.int32(s.N % 32)                   # bits past N: ignored
    region = torch.full((s.B, M), 0xA7, dtype=torch.uint8)                    # every bitmap's padding: ignored
    region[:, :W * 4] = torch.from_numpy(words.view(np.uint8).reshape(s.B, W * 4))
    region = region.reshape(-1).to(dev)
    far = torch.full((256, s.d), 10.0, dtype=s.Dd.dtype)                      # rows that would win every top-k if read
    Qd, qh = guarded_input(s.Qd.cpu(), tail=torch.full((128, s.d), 1e3, dtype=s.Qd.dtype))
    Dd, dh = guarded_input(s.Dd.cpu(), tail=far)
    fn = lib().gdr_sim_topk_bf16 if s.bf16 else lib().gdr_sim_topk
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill in (0x00, 0xFF, 0x5A):
        ws, hws = poisoned_workspace(need, fill, dev)
        ws[:s.B * M].copy_(region)
        v, hv = guarded((s.B, s.k), torch.float32, dev)
        i, hi = guarded((s.B, s.k), torch.int32, dev)
        st, hst = guarded((s.B,), torch.int32, dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        for rep in range(2 if fill == 0x5A else 1):                           # the last fill runs twice on the warm workspace
            with torch.cuda.stream(side):
                assert stream_ptr().value == side.cuda_stream and side.cuda_stream != 0
                rc = fn(ptr(Qd), s.B, ptr(Dd), s.N, s.d, s.k, 0, ptr(v), ptr(i), ptr(st), flags, ptr(ws), need, stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            side.synchronize()
            tag = f"{form} fill 0x{fill:02X} run {rep}"
            for h, name in ((hws, "workspace"), (hv, "out_val"), (hi, "out_idx"), (hst, "status")):
                h.check(f"{tag}: {name}")
            assert torch.equal(ws[:s.B * M], region), f"{tag}: the bitmap region was written"
            runs.append((v.clone(), i.clone(), st.clone()))
    qh.unchanged("Q")
    dh.unchanged("D")
    assert lib().gdr_device_fault_pending() == 0
    for v, i, st in runs:
        assert int(st.abs().sum()) == 0
        assert torch.equal(v, runs[0][0]) and torch.equal(i, runs[0][1]), "the result depends on what the scratch held"
    _check_raw(s, a, set(), *runs[0], form)
    _check_exact(s, a, runs[0][0], runs[0][1], form)


@pytest.mark.parametrize("form", ["tiled_B40", "stream_B4", "deep_select_B4"])
def test_two_runs_are_bit_identical(dev, form):
    s = _data(form, dev)
    a, _ = _allowed(s, "halves", None)
    x, y = _raw(s.Qd, s.Dd, s.k, s.flags, allowed=a), _raw(s.Qd, s.Dd, s.k, s.flags, allowed=a)
    assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_filtered_call_in_a_captured_graph(dev):
    """One filtered call captured in a graph — the strided copy of the bitmaps into the workspace, the passes, the mask launches
    and the per-query fix-up — replayed; then the QueryRows changes in place, and the replay follows it."""
    s = _data("tiled_B40", dev)
    a, _ = _allowed(s, "halves", None)
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, s.flags | QM)
    ws = live_ref.FixedWorkspace(torch.empty(need, dtype=torch.uint8, device=dev))
    call = lambda: ops.sim_topk(s.Qd, s.Dd, s.k, workspace=ws, flags=s.flags, allowed=R, exact_on_overflow=False, return_status=True)   # noqa: E731
    warm = torch.cuda.Stream(device=dev)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ev, ei, est = call()                                                  # eager; also the one run a capture needs first
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    ev, ei = ev.clone(), ei.clone()
    assert int(est.abs().sum()) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv, gi, gst = call()
    gv.zero_(), gi.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gv, ev) and torch.equal(gi, ei) and int(gst.abs().sum()) == 0
    _check_exact(s, a, gv, gi, "graph replay")
    got = ei.cpu().numpy()
    for q in range(s.B):                                                      # every query is now denied what it was just given
        a[q, got[q]] = False
    R.words.copy_(ops.QueryRows.from_bool(torch.from_numpy(a).to(dev)).words)
    g.replay()
    torch.cuda.synchronize()
    after = gi.cpu().numpy()
    assert not any(np.isin(after[q], got[q]).any() for q in range(s.B)) and int(gst.abs().sum()) == 0
    _check_exact(s, a, gv, gi, "graph replay after the filters changed")


def test_live_and_allowed_together_are_their_and(dev):
    s = _data("tiled_B40", dev)
    a, _ = _allowed(s, "halves", None)
    live = np.random.default_rng(21).random(s.N) < 0.8
    live[s.i0.cpu().numpy()[:, 0]] = False                                    # every query's best row is dead
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    bv, bi = ops.sim_topk(s.Qd, s.Dd, s.k, live=L, allowed=R)
    assert np.array_equal(R.to_bool().cpu().numpy(), a), "sim_topk must not change the caller's QueryRows"
    both = R.rows(torch.arange(s.B)).and_(L)
    av, ai = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=both)
    assert torch.equal(bv, av) and torch.equal(bi, ai)
    _check_exact(s, a & live, bv, bi, "live= and allowed=")
    pv, pi = ops.sim_topk(s.Qd, ops.PrefilteredCorpus(s.Dd), s.k, allowed=both)   # the pre-filter has no mask: the plain fp32 path
    assert torch.equal(pv, av) and torch.equal(pi, ai)
    with pytest.raises(_ffi.GdrError, match="QueryRows of 40 queries over the 20000 rows"):
        ops.sim_topk(s.Qd, s.Dd, s.k, allowed=ops.QueryRows(39, s.N, dev))
    with pytest.raises(_ffi.GdrError, match="QueryRows of 40 queries over the 20000 rows"):
        ops.sim_topk(s.Qd, s.Dd, s.k, allowed=ops.QueryRows(40, s.N - 1, dev))
    # the C call refuses both layouts at once
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, QM)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib().gdr_sim_topk(ptr(s.Qd), s.B, ptr(s.Dd), s.N, s.d, s.k, 0, ptr(bv), ptr(bi), None, LIVE | QM, ptr(ws), need, stream_ptr())
    assert rc == _ffi.GDR_EINVAL and b"GDR_SIM_QUERY_MASK" in lib().gdr_last_error()


# ------------------------------------------------------------------------------------------------ the retriever
def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=4, length_penalty=0.8, kary=V,
                                 position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_retriever_search_with_a_filter_after_remove_documents(dev):
    """A removed document that a query's filter allows does not come back: GDRRetriever.search ANDs the filter with live_rows, and
    the result is DenseModel.search's with the ANDed rows."""
    from gdr_amd.modeling import DenseModel, GDRRetriever
    V, csz, d, k, B = 30, 3, 64, 20, 6
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N = len(names) * csz
    D0 = synth.make_corpus(N, d, cluster_size=csz, seed=8)
    Q, _ = synth.make_queries(D0, B, seed=3)
    Qd = torch.from_numpy(Q).to(dev)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N, dtype=np.int32))
    r = GDRRetriever(None, torch.from_numpy(D0).to(dev), idx, _args(V))
    dense = DenseModel(None)
    S = live_ref.scores(Q, D0)
    base = r.search(Qd, k)[1].cpu().numpy()
    gone = np.unique(np.concatenate([base[:, :5].reshape(-1), np.arange(0, N, 7)]))
    offs, mem, n = lifecycle_ref.remove(idx.offsets, idx.members, gone)
    assert r.remove_documents(gone) == n
    live = np.zeros(N, bool)
    live[np.asarray(mem)] = True
    a = np.random.default_rng(4).random((B, N)) < 0.5
    for q in range(B):
        a[q, base[q, :10]] = True                                             # allowed by the filter; the first five are removed
        a[q, base[q, 10:]] = q % 2 == 0                                       # odd queries are denied the rest of their old list
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    v, i = r.search(Qd, k, allowed=R)
    assert i.dtype == torch.int64 and np.array_equal(R.to_bool().cpu().numpy(), a)
    got = i.cpu().numpy()
    assert not np.isin(got, gone).any(), "a removed document that the filter allows came back"
    for q in range(B):
        kept = base[q][~np.isin(base[q], gone)]                               # what is left of the old list
        assert kept.size and np.isin(kept, got[q]).sum() == (kept.size if q % 2 == 0 else np.isin(kept, base[q, :10]).sum())
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    fv, fi = dense.search(Qd, r.doc_embed, k, allowed=R.rows(torch.arange(B)).and_(L))
    assert torch.equal(v, fv) and torch.equal(i, fi)
    lv, li = dense.search(Qd, r.doc_embed, k, live=L, allowed=R)
    assert torch.equal(v, lv) and torch.equal(i, li)
    s = types.SimpleNamespace(S=S, B=B, k=k)
    _check_exact(s, a & live, v, i.to(torch.int32), "GDRRetriever.search(allowed=)")
    sh = GDRRetriever(None, r.doc_embed, r.index, _args(V), sharded=types.SimpleNamespace(D=r.doc_embed))
    with pytest.raises(_ffi.GdrError, match="sharded"):
        sh.search(Qd, k, allowed=R)
