"""The in-cluster rerank beyond 8192 candidates per query (DESIGN.md §4 "Rerank beyond 8192 candidates"): the chunked select
(GDR_RERANK_CHUNKED / max_cand > 8192) against the one-sort select bit for bit, long lists against an expectation assembled
from one-sort calls, against the oracle, and through block_max_cand / ShardedIndex / GDRRetriever."""
import types

import numpy as np
import pytest
import torch

from conftest import ranked_lists_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd.config import GDRConfig
from test_gpu_rerank import _rows_for

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = 1e-4
CH = ops.RERANK_CHUNK
ALPHAS9 = [0, 0.5, 1, 1.5, 2, 2.5, 3, 0.25, 0.75]               # more alphas than the partial-list scratch has slots (8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _split(rng, total, R, empty=()):
    """R uneven segment lengths that sum to `total`, the segments in `empty` (and others, when total is small) empty."""
    w = rng.random(R) ** 2 + 0.05
    w[list(empty)] = 0
    lens = np.floor(w / w.sum() * total).astype(np.int64)
    lens[int(np.argmax(w))] += total - lens.sum()
    assert lens.sum() == total and (lens >= 0).all()
    return lens


def _layouts(segs, dev, stride=None):
    """segs[b][j] = int32 doc ids of segment j of query b -> {"one_csr": (offsets, ids, 0), "query_blocks": (offsets, ids, stride)}."""
    B, R = len(segs), len(segs[0])
    lens = np.array([[len(s) for s in row] for row in segs], np.int64)
    flat = np.concatenate([np.concatenate(row) for row in segs]).astype(np.int32)
    csr = np.concatenate([[0], np.cumsum(lens.reshape(-1))]).astype(np.int32)
    stride = stride or int(lens.sum(1).max()) + 37                  # cand_stride > max_cand
    offs = np.zeros((B, R + 1), np.int32)
    offs[:, 1:] = np.cumsum(lens, 1)
    blocks = np.full((B, stride), -7, np.int32)                     # never read: behind every query's live part
    for b, row in enumerate(segs):
        blocks[b, :offs[b, R]] = np.concatenate(row)
    up = lambda a: torch.from_numpy(a).to(dev)                      # noqa: E731
    return {"one_csr": (up(csr), up(flat if flat.size else np.zeros(1, np.int32)), 0), "query_blocks": (up(offs), up(blocks), stride)}


def _corpus(dev, N, d, seed, dup=None):
    D = synth.make_corpus(N, d, seed=seed)
    if dup is not None:
        D[dup[0]:dup[1]] = D[dup[0]]                                # exact copies of one row: exactly tied scores
    Dd = torch.from_numpy(D).to(dev)
    return D, {False: Dd, True: ops.to_bf16(Dd)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the chunked form equals the one-sort form, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_case(dev):
    """One batch with every count at which the chunk pass or the merge changes shape, a query with more candidates than
    max_cand (two, in fact: 2*CH+1 and 9000 against max_cand = 8192), a query without candidates, and 3*CH exact copies of
    one corpus row spread over the lists: about 40 % of all candidates tie exactly, across chunks and across segments."""
    N, d, R = 30000, 64, 12
    rng = np.random.default_rng(41)
    dup = (5000, 5000 + 3 * CH)
    counts = [0, 1, CH - 1, CH, CH + 1, 2 * CH + 1, 8191, 8192, 9000]
    segs = []
    for n in counts:
        lens = _split(rng, n, R, empty=(3,))
        ids = rng.integers(0, N, n).astype(np.int32)
        segs.append(np.split(ids, np.cumsum(lens)[:-1]))
    assert sum(int(((s >= dup[0]) & (s < dup[1])).sum() > 0) for s in segs[7]) >= 4           # copies in several segments
    allc = np.concatenate(segs[7])
    assert all(((allc[c * CH:(c + 1) * CH] >= dup[0]) & (allc[c * CH:(c + 1) * CH] < dup[1])).any() for c in range(2))
    D, Dd = _corpus(dev, N, d, 3, dup)
    Q, gold = synth.make_queries(D, len(counts), seed=4)
    unit = lambda x: x / np.linalg.norm(x)                          # noqa: E731
    Q[7] += np.float32(5 / 3) * (unit(D[dup[0]]) - unit(D[gold[7]]))   # query 7's gold doc is the copied row: the copies rank first
    Q *= 0.15
    beam = np.sort(rng.standard_normal((len(counts), R)).astype(np.float32) * 2 - 8, axis=1)[:, ::-1].copy()
    return types.SimpleNamespace(N=N, R=R, B=len(counts), counts=counts, segs=segs, D=Dd, lay=_layouts(segs, dev),
                                 Q=torch.from_numpy(Q).to(dev), beam=torch.from_numpy(beam).to(dev))


@pytest.mark.parametrize("layout", ["one_csr", "query_blocks"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_chunked_equals_one_sort_bit_for_bit(dev, short_case, layout, bf16):
    s = short_case
    offs, ids, stride = s.lay[layout]
    assert stride == 0 or stride > ops.RERANK_MAX_CAND
    for func in ("tanh", "sigmoid"):
        for positions in (False, True):
            for k in (1, 100, 1024):
                kw = dict(func=func, max_cand=ops.RERANK_MAX_CAND, cand_stride=stride, positions=positions)
                v0, i0 = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, ALPHAS9, k, **kw)
                v1, i1 = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, ALPHAS9, k, chunked=True, **kw)
                assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1), (func, positions, k)
                live = (i0 >= 0).sum(-1).cpu().numpy()                                    # [B, A]: the padding was compared too
                want = np.minimum(np.minimum(s.counts, ops.RERANK_MAX_CAND), k)
                assert (live == want[:, None]).all(), (func, positions, k)
    # exact ties: with alpha = 0 the copies of one row are ranked by position alone (values equal, positions ascending)
    v, p = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, [0.0], 1024, max_cand=ops.RERANK_MAX_CAND, cand_stride=stride,
                           positions=True, chunked=True)
    v, p = v[7, 0].cpu().numpy(), p[7, 0].cpu().numpy()
    same = v[1:] == v[:-1]
    assert same.sum() > 100 and (p[1:][same] > p[:-1][same]).all()
    # a smaller max_cand than some lists (the surplus is ignored) and a width the chunk pass sorts in fewer than CH keys
    for mc in (1, 700, CH + 5):
        kw = dict(max_cand=mc, cand_stride=stride)
        v0, i0 = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, [0, 1.5], 100, **kw)
        v1, i1 = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, [0, 1.5], 100, chunked=True, **kw)
        assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1), mc
        assert int((i0[8] >= 0).sum()) == 2 * min(mc, 100)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_chunked_with_a_doc_range_that_empties_whole_chunks(dev, short_case, bf16):
    """A shard's row range: candidates outside it arrive as -inf and get no key.  Query 0's first chunk and query 1's second
    chunk hold no row of the shard at all; query 2 has no candidate inside it."""
    s = short_case
    lo, hi = 12000, 21000
    rng = np.random.default_rng(43)
    inside = lambda n: rng.integers(lo, hi, n).astype(np.int32)                       # noqa: E731
    outside = lambda n: rng.integers(0, lo, n).astype(np.int32)                       # noqa: E731
    lists = [np.concatenate([outside(CH), inside(900), outside(1000), inside(CH - 1900)]),
             np.concatenate([inside(CH), outside(CH)]),
             outside(CH + 10),
             np.concatenate([outside(50), inside(3), outside(50)])]
    segs = [np.split(x, np.cumsum(_split(rng, len(x), s.R))[:-1]) for x in lists]
    B = len(lists)
    for layout, (offs, ids, stride) in _layouts(segs, dev).items():
        kw = dict(max_cand=2 * CH, cand_stride=stride, doc_range=(lo, hi))
        for positions in (False, True):
            v0, i0 = ops.rerank_topk(s.Q[:B], s.D[bf16][lo:hi], offs, ids, s.beam[:B], ALPHAS9[:3], 100, positions=positions, **kw)
            v1, i1 = ops.rerank_topk(s.Q[:B], s.D[bf16][lo:hi], offs, ids, s.beam[:B], ALPHAS9[:3], 100, positions=positions,
                                     chunked=True, **kw)
            assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1), (layout, positions)
        assert (i0[:, 0] >= 0).sum(-1).tolist() == [100, 100, 0, 3]
        assert int(i0[0, 0].min()) >= CH                                               # positions: none from the empty chunk


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_8_shards_chunked_and_merged_equal_the_unsharded_one_sort_list(dev, short_case, bf16):
    """As test_gpu_rerank.test_rerank_8_shards_merged_is_bit_identical_to_unsharded, with the chunked form on every shard."""
    s = short_case
    offs, ids, stride = s.lay["query_blocks"]
    k, G, alphas = 25, 8, [0, 0.5, 2]
    A = len(alphas)
    kw = dict(max_cand=ops.RERANK_MAX_CAND, cand_stride=stride)
    v0, i0 = ops.rerank_topk(s.Q, s.D[bf16], offs, ids, s.beam, alphas, k, **kw)
    bounds = np.linspace(0, s.N, G + 1).astype(int)
    packs = []
    for g in range(G):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        vg, pg = ops.rerank_topk(s.Q, s.D[bf16][lo:hi], offs, ids, s.beam, alphas, k, doc_range=(lo, hi), positions=True,
                                 chunked=True, **kw)
        packs.append(ops.topk_pack(vg.view(s.B * A, k), pg.view(s.B * A, k)))
    mv, mp = ops.topk_merge_packed(torch.stack(packs))
    mi = ops.rerank_positions_to_ids(mp.view(s.B, A * k), ids).view(s.B, A, k)
    assert torch.equal(mv.view(s.B, A, k).view(torch.int32), v0.view(torch.int32)) and torch.equal(mi, i0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. long lists: exact, the expectation assembled from one-sort calls
# ---------------------------------------------------------------------------------------------------------------------
def _orderable(v):
    u = v.view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)                    # csrc/select.h fkey


def _expected_from_one_sort(Q, D, segs, beam, alphas, k, dev):
    """The R segments of every query are cut into groups of consecutive segments with at most 8192 candidates; the one-sort form
    ranks each group alone (same q, same R beam scores, the other segments empty: the softmax sees the same R scores, so every
    key has the same bits) and reports positions; a host merge by (key descending, global position ascending) gives the list."""
    B, R, A = len(segs), len(segs[0]), len(alphas)
    groups = []
    for row in segs:
        g, cur, n = [], [], 0
        for j, sgm in enumerate(row):
            if n + len(sgm) > ops.RERANK_MAX_CAND:
                g.append(cur)
                cur, n = [], 0
            cur.append(j)
            n += len(sgm)
        g.append(cur)
        groups.append(g)
    starts = [np.concatenate([[0], np.cumsum([len(x) for x in row])]) for row in segs]
    vals = [[[] for _ in range(A)] for _ in range(B)]
    poss = [[[] for _ in range(A)] for _ in range(B)]
    empty = np.zeros(0, np.int32)
    for gi in range(max(len(g) for g in groups)):
        part = [[(sgm if gi < len(groups[b]) and j in groups[b][gi] else empty) for j, sgm in enumerate(row)]
                for b, row in enumerate(segs)]
        offs, ids, stride = _layouts(part, dev, stride=ops.RERANK_MAX_CAND)["query_blocks"]
        v, p = ops.rerank_topk(Q, D, offs, ids, beam, alphas, k, max_cand=ops.RERANK_MAX_CAND, cand_stride=stride, positions=True)
        v, p = v.cpu().numpy(), p.cpu().numpy()
        for b in range(B):
            if gi >= len(groups[b]):
                assert (p[b] == -1).all()
                continue
            first = int(starts[b][groups[b][gi][0]])
            for a in range(A):
                live = p[b, a] >= 0
                vals[b][a].append(v[b, a][live])
                poss[b][a].append(p[b, a][live].astype(np.int64) + first)
    ev = np.full((B, A, k), -np.inf, np.float32)
    ep = np.full((B, A, k), -1, np.int32)
    for b in range(B):
        for a in range(A):
            v, p = np.concatenate(vals[b][a]), np.concatenate(poss[b][a])
            order = np.lexsort((p, -_orderable(v)))[:k]
            ev[b, a, :len(order)], ep[b, a, :len(order)] = v[order], p[order]
    return ev, ep, max(len(g) for g in groups)


@pytest.fixture(scope="module")
def long_case(dev):
    N, d, R = 60000, 64, 100
    rng = np.random.default_rng(47)
    counts = [8193, 10_000, 9 * CH + 5, 300]                       # the last: a short list inside a long batch, fewer than k = 1024
    segs = []
    for n in counts:
        lens = _split(rng, n, R, empty=(0, 17, 18, 99))
        ids = rng.integers(0, N, n).astype(np.int32)
        row = np.split(ids, np.cumsum(lens)[:-1])
        for j in (2, 40, 41, 77):                                  # one doc id repeated in several segments
            if len(row[j]):
                row[j][len(row[j]) // 2] = 1234
        segs.append(row)
    D, Dd = _corpus(dev, N, d, 13, dup=(20000, 20000 + 2 * CH))   # a third of the corpus ties exactly
    Q, _ = synth.make_queries(D, len(counts), seed=14)
    Q *= 0.15
    beam = np.sort(rng.standard_normal((len(counts), R)).astype(np.float32) * 2 - 8, axis=1)[:, ::-1].copy()
    return types.SimpleNamespace(counts=counts, segs=segs, D=Dd, Q=torch.from_numpy(Q).to(dev), beam=torch.from_numpy(beam).to(dev),
                                 lay=_layouts(segs, dev), flat=[np.concatenate(r) for r in segs])


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [100, 1024])
def test_long_lists_equal_the_merge_of_one_sort_groups_exactly(dev, long_case, k, bf16):
    s = long_case
    alphas = [0, 0.5, 3]
    B = len(s.counts)
    ev, ep, ngroups = _expected_from_one_sort(s.Q, s.D[bf16], s.segs, s.beam, alphas, k, dev)
    assert ngroups >= 5
    eid = np.stack([np.where(ep[b] >= 0, s.flat[b][np.maximum(ep[b], 0)], -1) for b in range(B)]).astype(np.int32)
    assert (np.sum(ep >= 0, -1) == np.minimum(s.counts, k)[:, None]).all()
    # max_cand = 9*CH+5: at k = 1024 a merge round takes 8 lists, so the 10 chunks need a second round; at k = 100 one round
    # serves.  max_cand = 10 000 (the first two queries): 3 chunks, one round at either k.
    lists_per_round = ops.RERANK_MAX_CAND // k
    assert (-(-(9 * CH + 5) // CH) > lists_per_round) == (k == 1024) and -(-10_000 // CH) <= lists_per_round
    for layout, (offs, ids, stride) in s.lay.items():
        for nq, mc in ((B, 9 * CH + 5), (2, 10_000)):
            o = offs if stride else offs[:nq * 100 + 1]
            for positions, want in ((True, ep), (False, eid)):
                v, i = ops.rerank_topk(s.Q[:nq], s.D[bf16], o, ids, s.beam[:nq], alphas, k, max_cand=mc, cand_stride=stride,
                                       positions=positions)
                assert np.array_equal(v.cpu().numpy().view(np.uint32), ev[:nq].view(np.uint32)), (layout, mc, positions)
                assert np.array_equal(i.cpu().numpy(), want[:nq]), (layout, mc, positions)


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_long_lists_vs_oracle(dev):
    from oracle import retrieval_ref
    N, d, B, R, k = 60000, 768, 2, 100, 100
    alphas = [0, 0.5, 1, 1.5, 2, 2.5, 3]
    rng = np.random.default_rng(53)
    counts = [10_007, 40_013]
    segs = [np.split(rng.choice(N, n, replace=False).astype(np.int32), np.cumsum(_split(rng, n, R, empty=(5,)))[:-1]) for n in counts]
    D = synth.make_corpus(N, d, seed=3)
    Q, _ = synth.make_queries(D, B, seed=4)
    Q *= 0.15                                                   # away from tanh saturation
    beam = np.sort(rng.standard_normal((B, R)).astype(np.float32) * 2 - 8, axis=1)[:, ::-1].copy()
    Qd, Dd, bd = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(beam).to(dev)
    lay = _layouts(segs, dev)
    offs, ids, stride = lay["query_blocks"]
    v, i = ops.rerank_topk(Qd, Dd, offs, ids, bd, alphas, k, max_cand=max(counts), cand_stride=stride)
    v2, i2 = ops.rerank_topk(Qd, Dd, lay["one_csr"][0], lay["one_csr"][1], bd, alphas, k)     # max_cand read from the CSR
    assert torch.equal(v, v2) and torch.equal(i, i2)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    Dt = torch.from_numpy(D)
    for b in range(B):
        mem = np.concatenate(segs[b]).tolist()
        ref = retrieval_ref.rerank(torch.from_numpy(Q[b:b + 1]), Dt, [mem], [[len(x) for x in segs[b]]], beam[b:b + 1].tolist(),
                                   alphas, k)[0]
        for a in range(len(alphas)):
            rv, ri = ref[a]
            np.testing.assert_allclose(v[b, a], rv.numpy(), rtol=TOL, atol=TOL)
            ranked_lists_match(ri.tolist(), rv.numpy(), i[b, a].tolist(), TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the composition the retriever runs: device candidates -> block_max_cand -> rerank; ShardedIndex.rerank_own
# ---------------------------------------------------------------------------------------------------------------------
def test_ten_beams_in_one_1000_document_cluster_are_reranked(dev):
    """test_gpu_rerank.test_one_oversized_cluster_does_not_break_the_step's index: the rows that decode the outlier ten times
    (10 000 candidates per query) were refused; with the long cap they are ranked."""
    from gdr_amd.dist import ShardedIndex
    from oracle import retrieval_ref
    V, ml, d, R, B = 30, 10, 64, 10, 4
    sizes = np.full(300, 12, np.int64)
    sizes[7] = 1000
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(offsets[-1])
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(300)]
    index = codec.ClusterIndex(names, offsets, np.arange(N, dtype=np.int32))
    rng = np.random.Generator(np.random.PCG64(3))
    D = synth.make_corpus(N, d, seed=3)
    Q, _ = synth.make_queries(D, B, seed=4)
    Q *= 0.3
    beam = np.sort(rng.standard_normal((B, R)).astype(np.float32), axis=1)[:, ::-1].copy()
    dci = ops.DeviceClusterIndex(index, dev, V)
    Qd, Dd, bd = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(beam).to(dev)
    picks = [7] * (B * R)
    picks[R:2 * R] = [7] * (R - 2) + [11, 12]                  # one query somewhat shorter: 8 024 candidates in a long batch
    rows = _rows_for(names, picks, V, ml, rng)
    _cl, offs, ids, stride = dci.candidates(torch.from_numpy(rows).to(dev), B, R)
    assert stride == R * 1000 > ops.RERANK_MAX_CAND
    with pytest.raises(_ffi.GdrError, match="at most 8192"):
        ops.block_max_cand(offs, R, stride)
    mc = ops.block_max_cand(offs, R, stride, cap=ops.RERANK_LONG_MAX_CAND)
    assert mc == 10_000
    with pytest.raises(_ffi.GdrError, match="at most 9999"):
        ops.block_max_cand(offs, R, stride, cap=9999)
    alphas = [0, 1.5]
    v, i = ops.rerank_topk(Qd, Dd, offs, ids, bd, alphas, R, max_cand=mc, cand_stride=stride)
    sv, si = ShardedIndex(Dd, 0).rerank_own(Qd, offs, ids, bd, alphas, R)
    assert torch.equal(sv, v) and torch.equal(si, i)
    dec = codec.dec_2d(codec.decode_token(rows, kary=V, output_vocab_size=V), R)
    mem = [[m for s_ in row for m in index[s_]] for row in dec]
    num = [[len(index[s_]) for s_ in row] for row in dec]
    assert [len(m) for m in mem] == [10_000, 8024, 10_000, 10_000]
    ref = retrieval_ref.rerank(torch.from_numpy(Q), torch.from_numpy(D), mem, num, beam.tolist(), alphas, R)
    for b in range(B):
        for a in range(2):
            np.testing.assert_allclose(v[b, a].cpu().numpy(), ref[b][a][0].numpy(), rtol=TOL, atol=TOL)
            ranked_lists_match(ref[b][a][1].tolist(), ref[b][a][0].numpy(), i[b, a].cpu().tolist(), TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 5. through GDRRetriever
# ---------------------------------------------------------------------------------------------------------------------
def _args(V, R):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=GDRConfig.tiny().max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")


@pytest.fixture(scope="module")
def tiny_model(dev):
    """A trie of exactly the 8 cluster names (all 6 first digits occur): 6 beams end in 6 distinct clusters."""
    from gdr_amd.modeling import GDRModel
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    V = cfg.output_vocab_size
    assert V == 6
    names = ["0-1", "1-4", "2-1", "3-4", "4-1", "5-4", "0-3", "1-2"]
    trie = codec.Trie.from_docids(names, V)
    model = GDRModel(cfg, sd, dev, trie=trie, prefix_trie=trie)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    batch = {"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)}
    enc_h, _ = ops.T5EncoderHandle(cfg, sd, dev).forward(batch["source_ids"], batch["source_mask"], want_pooled=False)
    return types.SimpleNamespace(cfg=cfg, V=V, names=names, model=model, batch=batch, q=enc_h[:, 0].cpu().numpy().astype(np.float64))


def _clustered_corpus(rng, sizes, d):
    """Rows around one random direction per cluster (the clusters far apart), rows of a cluster contiguous."""
    cent = rng.standard_normal((len(sizes), d)).astype(np.float32)
    rows = np.repeat(cent, sizes, axis=0) + 0.1 * rng.standard_normal((int(np.sum(sizes)), d)).astype(np.float32)
    return cent, (rows * np.float32(0.05)).astype(np.float32)


def _decoded_sizes(out, index):
    per_query = []
    for row in out["clusters"]:
        assert len(set(row)) == len(row) and all(name in index.lookup for name in row), row
        per_query.append(sum(len(index[name]) for name in row))
    return per_query


def test_retriever_steps_over_clusters_of_1400_documents(dev, tiny_model):
    from gdr_amd.modeling import GDRRetriever
    s = tiny_model
    R = 6
    rng = np.random.default_rng(61)
    sizes = rng.integers(1400, 1501, 8)
    _cent, D = _clustered_corpus(rng, sizes, s.cfg.d_model)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    index = codec.ClusterIndex(s.names, offs, rng.permutation(len(D)).astype(np.int32))
    Dd = torch.from_numpy(D).to(dev)
    out = GDRRetriever(s.model, Dd, index, _args(s.V, R)).validation_step_i(s.batch)
    assert all(n > ops.RERANK_MAX_CAND for n in _decoded_sizes(out, index))
    host = GDRRetriever(s.model, Dd, index, _args(s.V, R), device_candidates=False).validation_step_i(s.batch)
    assert [list(r) for r in host["clusters"]] == [list(r) for r in out["clusters"]]
    assert torch.equal(host["rerank_values"], out["rerank_values"]) and torch.equal(host["doc_id_tensor"], out["doc_id_tensor"])
    assert int(out["doc_id_tensor"].min()) >= 0 and bool(torch.isfinite(out["rerank_values"]).all())
    # alpha = 0: the values are the R largest tanh(q . d) over the members of the decoded clusters
    q = s.q
    for b in range(len(q)):
        mem = np.array([m for name in out["clusters"][b] for m in index[name]])
        sc = np.tanh(D[mem].astype(np.float64) @ q[b])
        np.testing.assert_allclose(out["rerank_values"][b, 0].cpu().numpy(), np.sort(sc)[::-1][:R], rtol=TOL, atol=TOL)


def test_add_documents_grows_the_clusters_past_8192_candidates(dev, tiny_model):
    from gdr_amd.modeling import GDRRetriever
    s = tiny_model
    R = 6
    rng = np.random.default_rng(67)
    sizes = np.full(8, 1000)
    cent, D = _clustered_corpus(rng, sizes, s.cfg.d_model)
    N0 = len(D)
    index = codec.ClusterIndex(s.names, (np.arange(9) * 1000).astype(np.int32), np.arange(N0, dtype=np.int32))
    r = GDRRetriever(s.model, torch.from_numpy(D).to(dev), index, _args(s.V, R))
    before = r.validation_step_i(s.batch)
    assert all(n == 6000 for n in _decoded_sizes(before, r.index))                    # the one-sort path
    new = np.repeat(cent, 500, axis=0) + 0.1 * rng.standard_normal((8 * 500, cent.shape[1])).astype(np.float32)
    ids_new, cl_new = r.add_documents(torch.from_numpy((new * np.float32(0.05)).astype(np.float32)).to(dev))
    assert np.array_equal(cl_new, np.repeat(np.arange(8), 500)) and ids_new[0] == N0
    out = r.validation_step_i(s.batch)
    assert [list(x) for x in out["clusters"]] == [list(x) for x in before["clusters"]]
    assert all(n == 9000 for n in _decoded_sizes(out, r.index))                       # now the long path
    # every added id that a query's decoded clusters contain is among that query's candidates
    (dec, _sc), _ = s.model.generate(s.batch["source_ids"], attention_mask=s.batch["source_mask"],
                                     max_length=s.cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R,
                                     output_scores=True)
    B = s.batch["source_ids"].shape[0]
    _cl, offs, ids, stride = r._device_index().candidates(dec.to(dev), B, R)
    assert ops.block_max_cand(offs, R, stride, cap=ops.RERANK_LONG_MAX_CAND) == 9000
    offs, ids = offs.cpu().numpy(), ids.cpu().numpy()
    for b in range(B):
        added = {int(m) for name in out["clusters"][b] for m in r.index[name] if m >= N0}
        assert len(added) == 3000 and added <= set(ids[b, :offs[b, R]].tolist())
    # the step equals a retriever built on the grown corpus and index, and the host-CSR form of the same
    fresh = GDRRetriever(s.model, r.doc_embed.clone(), r.index, _args(s.V, R), device_candidates=False).validation_step_i(s.batch)
    assert torch.equal(fresh["rerank_values"], out["rerank_values"]) and torch.equal(fresh["doc_id_tensor"], out["doc_id_tensor"])
    assert int((out["doc_id_tensor"] >= N0).sum()) > 0                                # added documents are ranked
