"""Corpus expansion on the MI355X: gdr_cluster_centroids / nearest_cluster / gdr_cluster_insert against the
reference's golden (g14) and the host restatement (tests/expand_ref.py), GDRRetriever.add_documents end to end, and the CLI's
--expand_index / --save_index."""
import types

import numpy as np
import pytest
import torch

import expand_ref
from conftest import golden
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


def _g14():
    g = golden("g14_expand")
    idx = codec.ClusterIndex([str(x) for x in g["names"]], g["offsets"], g["members"])
    return g, idx, int(g["docnum"])


def _csr_index(rng, C, sizes, N):
    """C clusters of the given sizes over N rows (members distinct within a cluster, shuffled)."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mem = np.concatenate([rng.choice(N, s, replace=False) if s else np.zeros(0, np.int64) for s in sizes]).astype(np.int32)
    return codec.ClusterIndex(["c%d" % c for c in range(C)], offs, mem)


def test_centroids_bit_identical_to_reference_and_restatement(dev):
    g, idx, _ = _g14()
    cent, counts = ops.cluster_centroids(torch.from_numpy(g["D"]).to(dev), idx)
    assert np.array_equal(cent.cpu().numpy().view(np.uint32), g["ref_centroids"].view(np.uint32))
    assert np.array_equal(counts.cpu().numpy(), np.diff(g["offsets"]))
    # d = 768: 2,000 clusters of 1-200 members, one of more than 8k, two empty ones
    rng = np.random.default_rng(5)
    N = 20000
    sizes = np.concatenate([rng.integers(1, 201, 2000), [8300, 0, 0]])
    idx2 = _csr_index(rng, len(sizes), sizes, N)
    D = (rng.standard_normal((N, 768)) * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float32)
    cent, counts = ops.cluster_centroids(torch.from_numpy(D).to(dev), idx2)
    rc, rn = expand_ref.centroids(D, idx2.offsets, idx2.members)
    assert np.array_equal(counts.cpu().numpy(), rn)
    assert np.array_equal(cent.cpu().numpy().view(np.uint32), rc.view(np.uint32)), "centroids not bit-identical at d = 768"


def test_assignment_equals_golden_and_lies_within_the_fp32_band(dev):
    g, idx, docnum = _g14()
    D = torch.from_numpy(g["D"]).to(dev)
    cent, counts = ops.cluster_centroids(D, idx)
    tgt = ops.nearest_cluster(D[docnum:], cent, counts).cpu().numpy()
    rt, _gap, _band = expand_ref.assign(g["D"][docnum:], g["ref_centroids"], np.diff(g["offsets"]))
    assert np.array_equal(tgt, rt)
    exp = expand_ref.as_sets(g["exp_offsets"], g["exp_members"])
    for r, c in enumerate(tgt):
        assert docnum + r in exp[c]
    # 30k rows against 5k clusters at d = 768 (chunked: several gdr_sim_topk calls)
    rng = np.random.default_rng(7)
    C_ = 5000
    cen = rng.standard_normal((C_, 768)).astype(np.float32)
    cnt = rng.integers(1, 20, C_).astype(np.int32)
    cnt[rng.choice(C_, 300, replace=False)] = 0
    X = (cen[rng.integers(0, C_, 30000)] * 0.3 + rng.standard_normal((30000, 768))).astype(np.float32)
    got = ops.nearest_cluster(torch.from_numpy(X).to(dev), torch.from_numpy(cen).to(dev), torch.from_numpy(cnt).to(dev),
                              chunk=8192).cpu().numpy()
    assert (cnt[got] > 0).all(), "an empty cluster was chosen"
    *_, ok = expand_ref.assign(X, cen, cnt, choice=got)
    assert ok.all(), f"{int((~ok).sum())} choices outside the fp32 band of the maximum"


def test_merge_matches_restatement_and_is_deterministic(dev):
    rng = np.random.default_rng(11)
    C_, N = 600, 30000
    sizes = rng.integers(0, 40, C_)
    sizes[:5] = 0                                         # empty clusters
    sizes[11] = 5
    idx = _csr_index(rng, C_, sizes, N)
    n = 9000
    new_ids = np.arange(N, N + n, dtype=np.int32)
    tgt = rng.integers(5, C_, n).astype(np.int32)
    u = rng.random(n)
    tgt[u < 0.2] = 7                                      # one cluster receives > 1,000 (LDS sort)
    tgt[u > 0.45] = 9                                     # one receives > 4,096 (ordered compaction)
    tgt[tgt == 11] = 12                                   # a non-empty cluster that receives nothing
    assert sizes[11] > 0 and (tgt == 7).sum() > 1000 and (tgt == 9).sum() > 4096
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    want_o, want_m = expand_ref.merge(idx.offsets, idx.members, new_ids, tgt)
    runs = []
    for _ in range(2):
        o, m, mx = ops.cluster_insert(up(idx.offsets), up(idx.members), up(new_ids), up(tgt))
        runs.append((o.cpu().numpy(), m.cpu().numpy(), mx))
    for o, m, mx in runs:
        assert np.array_equal(o, want_o) and np.array_equal(m, want_m), "merged CSR differs from the restatement"
        assert mx == int(np.diff(want_o).max())
    # through a compact -> cluster map, as the assignment hands it over
    cmap = np.arange(5, C_, dtype=np.int32)               # the targets never name clusters 0-4
    inv = np.full(C_, -1, np.int32)
    inv[cmap] = np.arange(cmap.size)
    assert (inv[tgt] >= 0).all()
    o, m, _ = ops.cluster_insert(up(idx.offsets), up(idx.members), up(new_ids), up(inv[tgt]), target_map=up(cmap))
    assert np.array_equal(o.cpu().numpy(), want_o) and np.array_equal(m.cpu().numpy(), want_m)
    with pytest.raises(_ffi.GdrError):                    # a target outside the map: reported, not written
        ops.cluster_insert(up(idx.offsets), up(idx.members), up(new_ids[:3]), up([0, cmap.size, 1]), target_map=up(cmap))


def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=GDRConfig.tiny().max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_add_documents_in_three_calls_equals_one(dev):
    from gdr_amd.modeling import GDRRetriever
    g, idx, docnum = _g14()
    D = torch.from_numpy(g["D"]).to(dev)
    one = GDRRetriever(None, D[:docnum].clone(), idx, _args(30))
    ids1, cl1 = one.add_documents(D[docnum:])
    three = GDRRetriever(None, D[:docnum].clone(), idx, _args(30))
    parts = [three.add_documents(D[lo:hi]) for lo, hi in ((docnum, docnum + 1), (docnum + 1, docnum + 14),
                                                          (docnum + 14, D.shape[0]))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), ids1) and np.array_equal(ids1, np.arange(docnum, D.shape[0]))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), cl1)
    for r in (one, three):
        assert torch.equal(r.doc_embed, D)
        assert expand_ref.as_sets(r.index.offsets, r.index.members) == expand_ref.as_sets(g["exp_offsets"], g["exp_members"])
        dci = r._device_index()
        assert np.array_equal(dci.offsets.cpu().numpy(), r.index.offsets)
        assert np.array_equal(dci.members[:dci.n_members].cpu().numpy(), r.index.members)
        assert dci.max_cluster == int(np.diff(r.index.offsets).max())
    assert np.array_equal(one.index.offsets, three.index.offsets) and np.array_equal(one.index.members, three.index.members)


def test_assignment_does_not_depend_on_the_rows_in_the_call(dev):
    """d = 768: a row's cluster and its top-1 score are the same bits whether it is assigned alone, in a call of 13 rows or in
    one of hundreds (gdr_sim_topk would take the stream kernel at <= 32 rows, which sums K in another order).  Then the same
    through add_documents: 1, then 13, then the remaining rows give the index and doc_embed of one call."""
    from gdr_amd.modeling import GDRRetriever
    rng = np.random.default_rng(13)
    N0, C_, n = 24000, 2000, 600
    sizes = np.full(C_, N0 // C_)
    idx = codec.ClusterIndex(["%d-%d-%d" % (c // 900, c // 30 % 30, c % 30) for c in range(C_)],
                             np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), rng.permutation(N0).astype(np.int32))
    D0 = torch.from_numpy(rng.standard_normal((N0, 768)).astype(np.float32)).to(dev)
    X = torch.from_numpy(rng.standard_normal((n, 768)).astype(np.float32)).to(dev)
    fc = ops.FrozenCentroids(D0, idx)
    c_all, v_all = fc.assign(X, return_scores=True)
    parts = [fc.assign(X[lo:hi], return_scores=True) for lo, hi in ((0, 1), (1, 14), (14, 46), (46, n))]
    v_parts = torch.cat([p[1] for p in parts])
    assert torch.equal(v_parts.view(torch.int32), v_all.view(torch.int32)), "top-1 scores depend on the rows in the call"
    assert torch.equal(torch.cat([p[0] for p in parts]), c_all)
    one = GDRRetriever(None, D0.clone(), idx, _args(30))
    ids1, cl1 = one.add_documents(X)
    three = GDRRetriever(None, D0.clone(), idx, _args(30))
    got = [three.add_documents(X[lo:hi]) for lo, hi in ((0, 1), (1, 14), (14, n))]
    assert np.array_equal(np.concatenate([g_[1] for g_ in got]), cl1) and np.array_equal(cl1, c_all.cpu().numpy())
    assert torch.equal(three.doc_embed, one.doc_embed)
    assert np.array_equal(one.index.offsets, three.index.offsets) and np.array_equal(one.index.members, three.index.members)


@pytest.fixture(scope="module")
def tiny_setup(dev):
    from gdr_amd.modeling import GDRModel
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    V = cfg.output_vocab_size
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    csz = 3
    N0 = len(names) * csz
    D0 = synth.make_corpus(N0, cfg.d_model, cluster_size=csz, seed=8) * np.float32(0.05)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N0, dtype=np.int32))
    full = codec.Trie.from_docids(names, V)
    model = GDRModel(cfg, sd, dev, trie=full, prefix_trie=full)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    batch = {"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)}
    enc_h, _ = ops.T5EncoderHandle(cfg, sd, dev).forward(batch["source_ids"], batch["source_mask"], want_pooled=False)
    return types.SimpleNamespace(cfg=cfg, V=V, idx=idx, D0=D0, model=model, batch=batch, q=enc_h[:, 0].cpu().numpy().astype(np.float64))


def _planted_docs(s, dev):
    """200 random new docs plus one planted next to query 0: it joins a cluster that query 0 decodes and has the largest q·d
    of that query's candidates."""
    from gdr_amd.modeling import GDRRetriever
    out = GDRRetriever(s.model, torch.from_numpy(s.D0).to(dev), s.idx, _args(s.V)).validation_step_i(s.batch)
    fc = ops.FrozenCentroids(torch.from_numpy(s.D0).to(dev), s.idx)
    cent = fc.centroids.cpu().numpy().astype(np.float64)
    q = s.q[0]
    cands = [m for name in out["clusters"][0] for m in s.idx[name]]
    best = max(float(s.D0[m] @ q) for m in cands)
    qh = q / np.linalg.norm(q)
    for name in out["clusters"][0]:
        c = s.idx.lookup.get(name)
        if c is None:
            continue
        for a in (64.0, 32.0, 16.0, 8.0, 4.0, 2.0, 1.0):
            for t in (0.1, 0.25, 0.5, 1.0, 2.0, 4.0):
                x = (a * cent[c] + t * qh).astype(np.float32)
                sc = cent @ x.astype(np.float64)
                top2 = np.sort(sc)[-2:]
                if np.argmax(sc) == c and top2[1] - top2[0] > 1e-3 * abs(top2[1]) and best + 0.5 < float(x @ q) < 6.0:
                    rng = np.random.default_rng(3)
                    extra = (s.D0[rng.integers(0, len(s.D0), 200)] + 1e-4 * rng.standard_normal((200, s.D0.shape[1]))).astype(np.float32)
                    return np.concatenate([extra, x[None]]), c
    raise AssertionError("no planted document found for query 0")


def test_validation_after_insertion_equals_fresh_retriever(dev, tiny_setup):
    """Fails without the feature: the planted document is only reachable once it has been inserted."""
    from gdr_amd.modeling import GDRRetriever
    s = tiny_setup
    new, c = _planted_docs(s, dev)
    r = GDRRetriever(s.model, torch.from_numpy(s.D0).to(dev), s.idx, _args(s.V))
    ids, cl = r.add_documents(torch.from_numpy(new).to(dev))
    planted = int(ids[-1])
    assert cl[-1] == c and planted == len(s.D0) + len(new) - 1
    out = r.validation_step_i(s.batch)
    fresh = GDRRetriever(s.model, torch.from_numpy(np.concatenate([s.D0, new])).to(dev), r.index, _args(s.V))
    ref = fresh.validation_step_i(s.batch)
    assert torch.equal(out["doc_id_tensor"], ref["doc_id_tensor"]) and torch.equal(out["rerank_values"], ref["rerank_values"])
    assert int(out["doc_id_tensor"][0, 0, 0]) == planted, "the planted document is not rank 1 for its query"
    # the host index (device_candidates=False) sees the same lists after the same insertion
    h = GDRRetriever(s.model, torch.from_numpy(s.D0).to(dev), s.idx, _args(s.V), device_candidates=False)
    h.add_documents(torch.from_numpy(new).to(dev))
    assert np.array_equal(h.index.offsets, r.index.offsets) and np.array_equal(h.index.members, r.index.members)
    ho = h.validation_step_i(s.batch)
    assert torch.equal(ho["doc_id_tensor"].cpu(), out["doc_id_tensor"].cpu())
    assert torch.equal(ho["rerank_values"].cpu(), out["rerank_values"].cpu())


def test_add_documents_from_tokens_equals_embeds(dev):
    from gdr_amd.modeling import EncoderModel, GDRRetriever
    bc = synth.bert_config(True)
    tower = EncoderModel.from_state_dict(bc, synth.make_bert_state_dict(bc, seed=77), dev)
    d = bc["hidden_size"]
    rng = np.random.default_rng(2)
    N0, C_ = 600, 50
    idx = codec.ClusterIndex(["%d-%d" % (c // 30, c % 30) for c in range(C_)], (np.arange(C_ + 1) * 12).astype(np.int32),
                             rng.permutation(N0).astype(np.int32))
    D0 = torch.from_numpy(rng.standard_normal((N0, d)).astype(np.float32)).to(dev)
    tok0, msk0 = (torch.from_numpy(a).to(dev) for a in synth.make_tokens(N0, L=24, vocab_hi=bc["vocab_size"], seed=4))
    tok, msk = (torch.from_numpy(a).to(dev) for a in synth.make_tokens(40, L=32, vocab_hi=bc["vocab_size"], seed=6))
    a = GDRRetriever(None, D0.clone(), idx, _args(30), doc_tower=tower)
    b = GDRRetriever(None, D0.clone(), idx, _args(30), doc_tower=tower)
    a.add_documents(tokens=(tok, msk))
    b.add_documents(embeds=tower(passage={"input_ids": tok, "attention_mask": msk}))
    assert torch.equal(a.doc_embed, b.doc_embed)
    assert np.array_equal(a.index.offsets, b.index.offsets) and np.array_equal(a.index.members, b.index.members)
    # with the re-encode path configured, tokens= is required and appended to doc_tokens
    r = GDRRetriever(None, D0.clone(), idx, _args(30), doc_tower=tower, doc_tokens=(tok0, msk0))
    with pytest.raises(_ffi.GdrError, match="tokens"):
        r.add_documents(embeds=b.doc_embed[N0:])
    r.add_documents(tokens=(tok, msk))
    assert r.doc_tokens[0].shape == (N0 + 40, 32) and torch.equal(r.doc_tokens[0][N0:], tok)
    assert torch.equal(r.doc_tokens[1][:N0, :24], msk0) and int(r.doc_tokens[1][:N0, 24:].abs().sum()) == 0
    assert torch.equal(r.doc_embed, a.doc_embed)
    ptr_t = r.doc_tokens[0].data_ptr()                    # a second add appends into the grown buffers: no corpus copy
    r.add_documents(tokens=(tok[:8, :20], msk[:8, :20]))
    assert r.doc_tokens[0].data_ptr() == ptr_t and r.doc_tokens[0].shape == (N0 + 48, 32)
    assert torch.equal(r.doc_tokens[0][N0 + 40:, :20], tok[:8, :20]) and int(r.doc_tokens[1][N0 + 40:, 20:].abs().sum()) == 0
    assert torch.equal(r.doc_tokens[0][:N0, :24], tok0)


def test_add_documents_refusals(dev):
    from gdr_amd.modeling import GDRRetriever
    g, idx, docnum = _g14()
    D = torch.from_numpy(g["D"]).to(dev)
    sh = GDRRetriever(None, D[:docnum], idx, _args(30), sharded=types.SimpleNamespace(D=D[:docnum]))
    with pytest.raises(_ffi.GdrError, match="sharded"):
        sh.add_documents(D[docnum:])
    bf = GDRRetriever(None, D[:docnum].to(torch.bfloat16), idx, _args(30))
    with pytest.raises(_ffi.GdrError, match="bf16"):
        bf.add_documents(D[docnum:])
    r = GDRRetriever(None, D[:docnum].clone(), idx, _args(30))
    with pytest.raises(_ffi.GdrError, match="embeds must be"):
        r.add_documents(D[docnum:, :32].contiguous())
    assert r.doc_embed.shape[0] == docnum and np.array_equal(r.index.members, idx.members)   # nothing changed


def test_cli_expand_index_writes_the_restated_index(dev, tmp_path):
    from gdr_amd import main as gmain
    cfg = GDRConfig.tiny()
    rng = np.random.default_rng(21)
    V, d = 30, 512                                        # --model_info small: d_model 512
    names = ["%d-%d" % (c // V, c % V) for c in range(90)]
    docnum, N = 540, 700
    sizes = np.full(len(names), docnum // len(names))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mem = rng.permutation(docnum).astype(np.int32)
    mem = np.concatenate([mem, [600, 650]]).astype(np.int32)  # two rows >= docnum already in a cluster: not re-inserted
    offs[-1] += 2
    base = rng.standard_normal((len(names), d)).astype(np.float32) * 2
    D = rng.standard_normal((N, d)).astype(np.float32)
    cl = np.repeat(np.arange(len(names)), sizes)
    D[mem[:docnum]] += base[cl]
    D[docnum:] += base[rng.integers(0, len(names), N - docnum)]
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    npz = tmp_path / "data.npz"
    np.savez(npz, source_ids=ids, source_mask=mask, gt_cluster=np.array(names[:4]), gt_doc=np.array(["1", "2", "3", "4"]),
             cluster_names=np.array(names), cluster_offsets=offs, cluster_members=mem)
    np.save(tmp_path / "doc.npy", D)
    base = ["--mode", "eval", "--model_info", "small", "--data_npz", str(npz), "--doc_embed_npy", str(tmp_path / "doc.npy"),
            "--num_return_sequences", "4", "--eval_batch_size", "4", "--max_output_length", "4", "--docnum", str(docnum),
            "--score_rate", "0", "1"]
    gmain.main(base + ["--res1_save_path", str(tmp_path / "plain.tsv")])
    gmain.main(base + ["--res1_save_path", str(tmp_path / "same.tsv"), "--save_index", str(tmp_path / "same.npz")])
    gmain.main(base + ["--res1_save_path", str(tmp_path / "exp.tsv"), "--expand_index", "1", "--save_index",
                       str(tmp_path / "exp.npz")])
    # without the flag: the index and the outputs are those of a run that does not know the flags
    z = np.load(tmp_path / "same.npz")
    assert np.array_equal(z["cluster_offsets"], offs) and np.array_equal(z["cluster_members"], mem)
    for suffix in ("", ".docs.tsv"):
        assert open(str(tmp_path / "plain.tsv") + suffix).read() == open(str(tmp_path / "same.tsv") + suffix).read()
    # with it: the restatement's index, names unchanged
    rows = np.setdiff1d(np.arange(docnum, N), mem)
    cent, counts = expand_ref.centroids(D, offs, mem)
    tgt, gap, band = expand_ref.assign(D[rows], cent, counts)
    assert (gap > band).all()
    want_o, want_m = expand_ref.merge(offs, mem, rows, tgt)
    z = np.load(tmp_path / "exp.npz")
    assert [str(x) for x in z["cluster_names"]] == names
    assert np.array_equal(z["cluster_offsets"], want_o) and np.array_equal(z["cluster_members"], want_m)
