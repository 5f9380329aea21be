"""Corpus-wide top-k of 1024 < k <= 8192 documents per query (gdr_sim_topk[_bf16], gdr_topk_merge, gdr_topk_pack,
gdr_topk_merge_packed; csrc/sim_topk.hip topk_select_kernel<.., DEEP>): the radix passes of the k <= 1024 select pick the keys, the
whole workgroup sorts them in LDS.  Every deep-k call here is GDR_EINVAL on the commit before.

Why the main oracle is EXACT: at this depth the usual tolerance rule cannot fail.  At synth.make_corpus(50000, 128, seed=21), 8
queries, k = 4096, about 3 150 of the 4 095 neighbouring float64 scores lie closer than twice the fp32 band
(2d + 8) 2^-24 |q| max|d| (~ 8e-5), so order_insensitive_topk_match at 1e-4 chains almost the whole list into one tie group.
Integer inputs in [-3, 3] make every product and partial sum an integer of magnitude <= 9 d <= 2304 < 2^24: every fp32 (and
bf16-operand, fp32-accumulate) score is exact in any summation order, and the expected list is np.lexsort((ids, -scores))[:k] —
the library's rule, higher score, then lower id — compared with torch.equal.  The float case measures its own window instead."""
import functools

import numpy as np
import pytest
import torch

from gdr_amd import _ffi, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


# ---- 1. exact lists on integer inputs ------------------------------------------------------------------------------------------
N_MAX, B_MAX = 140_001, 40


@functools.lru_cache(maxsize=None)
def _ints(d):
    g = np.random.default_rng(3)
    Q = g.integers(-3, 4, size=(B_MAX, d)).astype(np.float32)
    D = g.integers(-3, 4, size=(N_MAX if d == 128 else 70_001, d)).astype(np.float32)
    return Q, D


@functools.lru_cache(maxsize=None)
def _int_scores(d, N):
    Q, D = _ints(d)
    s = Q @ D[:N].T                                               # exact: integers below 2^24
    assert np.abs(s).max() <= 9 * d
    return s.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _int_expected(d, N, k):
    """(values fp32 [B_MAX,k], ids int32 [B_MAX,k]) by the library's rule, and per query how many docs tie with the cut inside / in all."""
    s = _int_scores(d, N)
    ids = np.arange(N)
    vals, idx, ties = [], [], []
    for q in range(s.shape[0]):
        order = np.lexsort((ids, -s[q]))[:k]
        vals.append(s[q, order]), idx.append(order)
        cut = s[q, order[-1]]
        ties.append((int((s[q, order] == cut).sum()), int((s[q] == cut).sum())))
    return torch.from_numpy(np.stack(vals).astype(np.float32)), torch.from_numpy(np.stack(idx).astype(np.int32)), ties


_DEV = {}


def _on_dev(key, make, dev):
    if key not in _DEV:
        _DEV[key] = make().to(dev)
    return _DEV[key]


def _run(Q, D, k, dev, flags=0, idx_offset=0):
    """the call under test, with the repair switched off: status must be 0, so that the path named in the table is what answered"""
    v, i, st = ops.sim_topk(Q, D, k, idx_offset=idx_offset, return_status=True, exact_on_overflow=False, flags=flags)
    assert int(st.sum()) == 0, "a candidate list overflowed"
    return v.cpu(), i.cpu()


# N, k, path make_plan gives it
INT_SHAPES = [(8_192, 8_192, "k == N"), (9_000, 8_192, "stride 1"), (70_001, 1_025, "stride 6, list over the register cache"),
              (70_001, 2_048, "stride 5"), (70_001, 4_097, "stride 4, kpad 8192"), (70_001, 8_192, "stride 1"),
              (140_001, 8_192, "stride 4, n_slots 35 072, cap 169 984")]


@pytest.mark.parametrize("N,k,path", INT_SHAPES, ids=[f"N{n}-k{k}" for n, k, _ in INT_SHAPES])
def test_integer_scores_give_the_exact_list(dev, N, k, path):
    d = 128
    Qn, Dn = _ints(d)
    ev, ei, ties = _int_expected(d, N, k)
    if N == 140_001:
        # the "lower id" rule at the cut is what is tested: some query's cut splits a tie group (checked before anything runs)
        print("docs tied with the cut (inside the list, in all), 4 queries:", ties[:4])
        assert any(inside < total for inside, total in ties[:3]), ties[:3]
    Q = _on_dev(("Q", d), lambda: torch.from_numpy(Qn), dev)
    D = _on_dev(("D", d), lambda: torch.from_numpy(Dn), dev)[:N]
    for what, B, flags in (("stream kernels", 3, 0), ("SIM_NO_STREAM", 3, _ffi.SIM_NO_STREAM), ("tiled core", 40, 0)):
        v, i = _run(Q[:B].contiguous(), D, k, dev, flags)
        assert torch.equal(i, ei[:B]), (path, what, "ids")
        assert torch.equal(v, ev[:B]), (path, what, "values")
    if N == 70_001 and k == 4_097:
        for B in (3, 40):
            v, i = _run(Q[:B].contiguous(), D, k, dev, idx_offset=1000)
            assert torch.equal(i, ei[:B] + 1000) and torch.equal(v, ev[:B]), (path, "idx_offset", B)


@pytest.mark.parametrize("k", [4_097, 8_192])
def test_integer_scores_bf16_corpus(dev, k):
    """components in [-3, 3] are exact in bf16: the bf16 path owes the same list"""
    d, N = 256, 70_001
    Qn, Dn = _ints(d)
    ev, ei, _ = _int_expected(d, N, k)
    Q = _on_dev(("Q", d), lambda: torch.from_numpy(Qn), dev)
    D16 = _on_dev(("D16", d), lambda: torch.from_numpy(Dn).bfloat16(), dev)
    assert torch.equal(D16.float().cpu(), torch.from_numpy(Dn))
    for B in (3, 40):
        v, i = _run(Q[:B].contiguous(), D16, k, dev)
        assert torch.equal(i, ei[:B]) and torch.equal(v, ev[:B]), B


# ---- 2. overflow at depth -------------------------------------------------------------------------------------------------------
def test_overflow_at_depth_is_flagged_and_repaired(dev):
    """70 001 identical rows: every doc reaches the sampled threshold, the list overflows.  Unrepaired: status 1.  Repaired (the
    default; the exhaustive re-run selects from a list of N entries, far over the register cache): ids 0 .. k-1, equal values.
    Asserted on the tiled core (SIM_NO_STREAM, and 40 queries), where one kernel form scores every row, so identical rows get
    identical bits.  The fp32 stream form (B <= 32) scores the sample tiles with its split-K kernel when there are at most 256 of
    them and the other tiles with its ring kernel — two summation orders, e.g. 0x1.51f432p+0 against 0x1.51f436p+0 for the same
    row — so a query whose sample scores come out above the others' never fills its list (measured: status [1, 1, 0]); there the
    call owes a repaired, well-formed list and nothing about which of the equal rows it names."""
    N, d, k = 70_001, 128, 2_048
    row = torch.from_numpy(synth.make_corpus(1, d, seed=5))
    D = row.repeat(N, 1).to(dev)
    Q = torch.from_numpy(synth.make_queries(row.numpy(), 40, seed=6)[0]).to(dev)
    for B, flags in ((3, _ffi.SIM_NO_STREAM), (40, 0)):
        q = Q[:B].contiguous()
        _, _, st = ops.sim_topk(q, D, k, exact_on_overflow=False, return_status=True, flags=flags)
        assert st.cpu().tolist() == [1] * B
        v, i, st = ops.sim_topk(q, D, k, return_status=True, flags=flags)
        assert st.cpu().tolist() == [0] * B
        assert torch.equal(i.cpu(), torch.arange(k, dtype=torch.int32).repeat(B, 1))
        assert bool((v == v[:, :1]).all())
    v, i, st = ops.sim_topk(Q[:3].contiguous(), D, k, return_status=True)          # the stream form
    assert st.cpu().tolist() == [0, 0, 0]
    i = i.cpu().sort(dim=1).values
    assert bool((i[:, 1:] > i[:, :-1]).all()) and int(i.min()) >= 0 and int(i.max()) < N
    band = (2 * d + 8) * 2.0 ** -24 * Q[:3].norm(dim=1) * float(row.norm())       # two fp32 sums of one row differ by at most 2 bands
    assert bool((v[:, 1:] <= v[:, :-1]).all()) and bool((v[:, 0] - v[:, -1] <= 2 * band).all())


# ---- 3. float inputs, with a measured window ------------------------------------------------------------------------------------
FN, FD, FB, FK = 50_000, 128, 8, 4_096


@functools.lru_cache(maxsize=None)
def _floats():
    D = synth.make_corpus(FN, FD, seed=21)
    Q, _ = synth.make_queries(D, FB)
    return Q, D


def _check_against_float64(v, i, Q64, D64, k):
    """e = max |gpu value - float64 score of the same id| <= the fp32 band; the ids follow the float64 order up to ties inside 2e."""
    s = Q64 @ D64.T                                               # [B, N] float64
    N = s.shape[1]
    ids = np.arange(N)
    v, i = v.numpy().astype(np.float64), i.numpy().astype(np.int64)
    dmax = np.linalg.norm(D64, axis=1).max()
    worst, sizes = 0.0, []
    for q in range(s.shape[0]):
        band = (2 * FD + 8) * 2.0 ** -24 * np.linalg.norm(Q64[q]) * dmax
        assert len(set(i[q].tolist())) == k and i[q].min() >= 0 and i[q].max() < N
        e = np.abs(v[q] - s[q, i[q]]).max()
        print(f"query {q}: e = {e:.3e} = {e / band:.4f} of the band {band:.3e}")
        assert e <= band, (q, e, band)
        worst = max(worst, e / band)
        w = 2 * e
        order = np.lexsort((ids, -s[q]))
        so = s[q, order]
        rank = np.empty(N, np.int64)
        rank[order] = ids
        group = np.concatenate([[0], np.cumsum((so[:-1] - so[1:]) > w)])      # chains of float64 neighbours closer than 2e
        pos = rank[i[q]]                                                       # where the float64 order has the GPU's rank-j id
        inside = pos < k
        assert np.array_equal(group[pos[inside]], group[np.arange(k)[inside]]), (q, "an id sits outside its float64 tie chain")
        assert np.all(so[k - 1] - so[pos[~inside]] <= w), (q, "an id from outside the float64 list does not tie with the cut")
        gs = np.bincount(group[:k] - group[0])
        sizes.append((int(gs.max()), int((gs == 1).sum()), int((~inside).sum())))
    print("per query (largest tie chain, singleton chains, ids from outside the float64 list):", sizes)
    # the rule can only fail where chains are short: most ranks must stand alone (a window of 2e is ~1e-6 against a mean gap of
    # (score range ~ 0.3) / k ~ 1e-4, so a rank is chained to its neighbour with probability ~1e-2)
    assert all(big <= k // 64 and single >= k // 2 for big, single, _ in sizes), sizes
    return worst


@pytest.mark.parametrize("corpus", ["fp32", "bf16"])
def test_float_scores_inside_the_measured_window(dev, corpus):
    Qn, Dn = _floats()
    Q, D = torch.from_numpy(Qn), torch.from_numpy(Dn)
    if corpus == "bf16":                                           # the device rounds the queries too: score against the widened operands
        Dd, Q64, D64 = D.bfloat16().to(dev), Q.bfloat16().double().numpy(), D.bfloat16().double().numpy()
    else:
        Dd, Q64, D64 = D.to(dev), Q.double().numpy(), D.double().numpy()
    v, i = _run(Q.to(dev), Dd, FK, dev)
    _check_against_float64(v, i, Q64, D64, FK)


# ---- 4. merges ------------------------------------------------------------------------------------------------------------------
def _shard_lists(G, B, k, seed, short):
    """per-shard sorted lists of integer scores with disjoint ids; `short` (query -> live entries per shard) leaves -inf / -1 padding"""
    g = np.random.default_rng(seed)
    vals = np.full((G, B, k), -np.inf, np.float32)
    idx = np.full((G, B, k), -1, np.int32)
    for s in range(G):
        for q in range(B):
            n = short.get(q, k)
            sc = g.integers(-40, 41, size=n)
            ids = s * 100_000 + g.choice(100_000, size=n, replace=False)
            o = np.lexsort((ids, -sc))
            vals[s, q, :n], idx[s, q, :n] = sc[o], ids[o]
    return vals, idx


def _merge_expected(vals, idx, k):
    G, B, _ = vals.shape
    ev = np.full((B, k), -np.inf, np.float32)
    ei = np.full((B, k), -1, np.int32)
    for q in range(B):
        live = idx[:, q].reshape(-1) >= 0
        sc, ids = vals[:, q].reshape(-1)[live], idx[:, q].reshape(-1)[live]
        o = np.lexsort((ids, -sc.astype(np.int64)))[:k]
        ev[q, :len(o)], ei[q, :len(o)] = sc[o], ids[o]
    return torch.from_numpy(ev), torch.from_numpy(ei)


@pytest.mark.parametrize("G,B,k,short", [(8, 5, 2_048, {1: 100, 3: 0}), (3, 2, 8_192, {1: 2_000})],
                         ids=["G8-B5-k2048", "G3-B2-k8192"])
def test_merges_at_depth(dev, G, B, k, short):
    """(8, 5, 2048): 16 384 keys per query, exactly the merge form's register cache (16 per thread).  Query 1 of
    the second case holds 6 000 live entries for k = 8192: the tail of its list is -inf / -1 padding; query 3 of the first has none."""
    vals, idx = _shard_lists(G, B, k, 11, short)
    ev, ei = _merge_expected(vals, idx, k)
    tv, ti = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    mv, mi = ops.topk_merge(tv, ti)
    assert torch.equal(mi.cpu(), ei) and torch.equal(mv.cpu(), ev)
    # the wire form, with a status word: shard 1 flags query 0
    st = torch.zeros((G, B), dtype=torch.int32, device=dev)
    st[1, 0] = 1
    pairs = torch.stack([ops.topk_pack(tv[s], ti[s], st[s]) for s in range(G)])
    assert pairs.shape == (G, B, k + 1) and pairs.dtype == torch.int64
    pv, pi, ps = ops.topk_merge_packed(pairs, return_status=True)
    assert torch.equal(pi.cpu(), ei) and torch.equal(pv.cpu(), ev)
    assert ps.cpu().tolist() == [1] + [0] * (B - 1)
    pv2, pi2 = ops.topk_merge_packed(torch.stack([ops.topk_pack(tv[s], ti[s]) for s in range(G)]))
    assert torch.equal(pi2.cpu(), ei) and torch.equal(pv2.cpu(), ev)


def test_eight_row_shards_merge_to_the_unsharded_list(dev):
    """A doc's score does not depend on the shard that computed it: the merged shard lists ARE the unsharded list, bit for bit — on
    the tiled core, as in the k = 100 case of tests/test_gpu_dist.py (48 queries there and here).  At B <= 32 the fp32 stream form
    scores sample tiles and the other tiles in two summation orders, and which tiles are sampled depends on the shard's size."""
    _, Dn = _floats()
    B, k, G = 48, FK, 8
    Q = torch.from_numpy(synth.make_queries(Dn, B, seed=5)[0]).to(dev)
    D = torch.from_numpy(Dn).to(dev)
    uv, ui = ops.sim_topk(Q, D, k)
    per = FN // G
    assert per >= k
    parts = [ops.sim_topk(Q, D[g * per:(g + 1) * per].contiguous(), k, idx_offset=g * per) for g in range(G)]
    mv, mi = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, ui) and torch.equal(mv, uv)
    pairs = torch.stack([ops.topk_pack(p[0], p[1]) for p in parts])
    pv, pi = ops.topk_merge_packed(pairs)
    assert torch.equal(pi, ui) and torch.equal(pv, uv)


# ---- 5. surface -----------------------------------------------------------------------------------------------------------------
def test_surface_dense_model_sharded_index_and_prefiltered_corpus(dev):
    from gdr_amd.dist import ShardedIndex
    from gdr_amd.modeling import DenseModel
    Qn, Dn = _floats()
    Q, D = torch.from_numpy(Qn).to(dev), torch.from_numpy(Dn).to(dev)
    pv, pi = ops.sim_topk(Q, D, 3_000)
    # DenseModel.search
    v, i = DenseModel(lm_q=None).search(Q, D, 3_000)
    assert i.dtype == torch.int64 and torch.equal(i, pi.to(torch.int64)) and torch.equal(v, pv)
    # a PrefilteredCorpus past PREFILTER_MAX_K is the plain fp32 call over its rows, bit for bit; at the limit it is still the pre-filter
    P = ops.PrefilteredCorpus(D)
    fv, fi = ops.sim_topk(Q, P, 3_000)
    assert torch.equal(fi, pi) and torch.equal(fv, pv)
    v, i = DenseModel(lm_q=None).search(Q, P, 3_000)
    assert torch.equal(i, pi.to(torch.int64)) and torch.equal(v, pv)
    assert ops.sim_topk(Q, P, ops.PREFILTER_MAX_K)[1].shape == (FB, ops.PREFILTER_MAX_K)
    with pytest.raises(_ffi.GdrError, match="8192"):
        ops.sim_topk(Q, D, ops.SIM_TOPK_MAX_K + 1)
    # ShardedIndex, one rank: the three searches, and the wire row of k + 1 entries through pack -> merge_packed
    k = 2_048
    sv, si = ops.sim_topk(Q, D, k, idx_offset=7)
    sh = ShardedIndex(D, 7)
    for got in (sh.search(Q, k, return_status=True), sh.search_own(Q, k, return_status=True), sh.search_own_async(Q, k).wait()):
        assert torch.equal(got[0], sv) and torch.equal(got[1], si) and int(got[2].sum()) == 0
    wire = sh.pack(sv, si, got[2])
    assert wire.shape == (FB, k + 1)
    wv, wi, ws = sh.merge_packed(wire.view(1, FB, k + 1))
    assert torch.equal(wv, sv) and torch.equal(wi, si) and int(ws.sum()) == 0
