"""Document removal and update on the MI355X: the removal mode of gdr_cluster_insert (new_target == NULL)
against the host restatement (tests/lifecycle_ref.py), its memory contract (tests/abi_guard.py), and
GDRRetriever.remove_documents / update_documents end to end against a fresh retriever built over the restated index.
Integers are compared exactly."""
import types

import numpy as np
import pytest
import torch

import expand_ref
import lifecycle_ref
from abi_guard import guarded, guarded_input, poisoned_workspace
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu

# one below, at and one above the wave (64 members per ballot) and the tile one wave has in flight (RM_TILE = 256), the empty and
# the one-member cluster, and one of many tiles
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 5000)
N_IDS = 8000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


def _index(seed=17):
    """The member CSR of the kernel tests: clusters of SIZES over a random permutation of a subset of [0, N_IDS), unsorted."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    mem = rng.permutation(N_IDS)[:offs[-1]].astype(np.int32)
    return rng, offs, mem


def _removal_lists(rng, offs, mem):
    seg = lambda c: mem[offs[c]:offs[c + 1]]   # noqa: E731
    absent = np.setdiff1d(np.arange(N_IDS), mem)
    big = seg(8)
    lists = {
        "one id": mem[[4000]],
        "first and last of a segment": np.array([seg(7)[0], seg(7)[-1]]),
        "64 ids of one cluster": big[100:164],
        "65 ids of one cluster": big[250:315],
        "a one-member cluster": seg(1),
        "every member of one cluster": seg(7),
        "every member of the big cluster": big,
        "every member of the index": mem,
        "half of the ids absent": np.concatenate([rng.choice(mem, 200, replace=False), rng.choice(absent, 200, replace=False)]),
        "3000 random ids": rng.choice(N_IDS, 3000, replace=False),
    }
    return {k: np.unique(v).astype(np.int32) for k, v in lists.items()}


def _up(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def test_removal_kernel_matches_restatement(dev):
    rng, offs, mem = _index()
    up = _up(dev)
    offs_d, mem_d = up(offs), up(mem)
    for what, ids in _removal_lists(rng, offs, mem).items():
        assert np.all(np.diff(ids) > 0)
        want_o, want_m, want_n = lifecycle_ref.remove(offs, mem, ids)
        o, m, mx, gone = ops.cluster_remove(offs_d, mem_d, up(ids))
        assert np.array_equal(o.cpu().numpy(), want_o), f"{what}: offsets differ from the restatement"
        assert np.array_equal(m.cpu().numpy(), want_m), f"{what}: members differ from the restatement"
        assert mx == int(np.diff(want_o).max()) and gone == want_n, f"{what}: largest cluster {mx}, removed {gone}"
    assert int(ops.cluster_remove(offs_d, mem_d, up(mem[np.argsort(mem)]))[0][-1]) == 0
    # inconsistent old offsets are reported, not followed
    bad = offs.copy()
    bad[3] = bad[4] + 1
    with pytest.raises(_ffi.GdrError, match="inconsistent"):
        ops.cluster_remove(up(bad), mem_d, up([5]))
    with pytest.raises(_ffi.GdrError, match="inconsistent"):
        ops.cluster_remove(offs_d, mem_d[:-1], up([5]))
    # strided views of the inputs are made contiguous, as in cluster_insert
    ids = np.unique(rng.choice(N_IDS, 500, replace=False)).astype(np.int32)
    two = torch.stack([up(ids), up(ids)], 1)
    o, m, mx, gone = ops.cluster_remove(offs_d, torch.stack([mem_d, mem_d], 1)[:, 0], two[:, 1])
    want_o, want_m, want_n = lifecycle_ref.remove(offs, mem, ids)
    assert np.array_equal(o.cpu().numpy(), want_o) and np.array_equal(m.cpu().numpy(), want_m) and gone == want_n


def test_removal_mode_memory_contract(dev):
    """Guard bands around every buffer, out_members of exactly n_old entries of which nothing beyond out_offsets[C] is written,
    a workspace of exactly gdr_cluster_insert_workspace_bytes(C) poisoned beforehand, a non-default stream."""
    rng, offs, mem = _index()
    Cn, n_old = len(SIZES), int(offs[-1])
    ids = _removal_lists(rng, offs, mem)["3000 random ids"]
    want_o, want_m, want_n = lifecycle_ref.remove(offs, mem, ids)
    n_left = n_old - want_n
    # behind each input: values that would change the answer if they were read
    Od, oh = guarded_input(torch.from_numpy(offs), tail=torch.full((256,), n_old + 100, dtype=torch.int32))
    Md, mh = guarded_input(torch.from_numpy(mem), tail=torch.from_numpy(np.setdiff1d(np.arange(N_IDS), ids)[:1024].astype(np.int32)))
    Id, ih = guarded_input(torch.from_numpy(ids), tail=torch.from_numpy(np.setdiff1d(mem, ids)[-1024:].astype(np.int32)))
    need = lib().gdr_cluster_insert_workspace_bytes(Cn)
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill in (0x00, 0xFF, 0x5A):
        o_off, hoff = guarded((Cn + 1,), torch.int32, dev)
        o_mem, hmem = guarded((n_old,), torch.int32, dev)
        o_max, hmax = guarded((1,), torch.int32, dev)
        ws, hws = poisoned_workspace(need, fill, dev)
        before = o_mem.clone()
        side.wait_stream(torch.cuda.current_stream(dev))
        for rep in range(2 if fill == 0x5A else 1):                  # the last fill runs twice on the warm workspace
            with torch.cuda.stream(side):
                assert stream_ptr().value == side.cuda_stream and side.cuda_stream != 0
                rc = lib().gdr_cluster_insert(ptr(Od), ptr(Md), Cn, n_old, ptr(Id), None, len(ids), None, 0, ptr(o_off), ptr(o_mem),
                                              ptr(o_max), ptr(ws), need, stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            side.synchronize()
            tag = f"fill 0x{fill:02X} run {rep}"
            for h, name in ((hoff, "out_offsets"), (hmem, "out_members"), (hmax, "out_max"), (hws, "workspace")):
                h.check(f"{tag}: {name}")
            assert int(o_off[Cn]) == n_left
            assert torch.equal(o_mem[n_left:], before[n_left:]), f"{tag}: out_members written beyond out_offsets[C]"
            runs.append((o_off.clone(), o_mem[:n_left].clone(), o_max.clone()))
    for h in (oh, mh, ih):
        h.unchanged("removal mode: an input")
    assert lib().gdr_device_fault_pending() == 0
    for o, m, x in runs:
        assert np.array_equal(o.cpu().numpy(), want_o) and np.array_equal(m.cpu().numpy(), want_m)
        assert int(x) == int(np.diff(want_o).max())


def test_removal_is_deterministic_and_composes(dev):
    rng, offs, mem = _index(seed=23)
    up = _up(dev)
    ids = np.unique(rng.choice(N_IDS, 3000, replace=False)).astype(np.int32)
    a = ops.cluster_remove(up(offs), up(mem), up(ids))
    b = ops.cluster_remove(up(offs), up(mem), up(ids))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    # in three calls = the union in one
    o, m, gone = up(offs), up(mem), 0
    for part in (ids[::3], ids[1::3], ids[2::3]):
        o, m, mx, g = ops.cluster_remove(o, m, up(part))
        gone += g
    assert torch.equal(o, a[0]) and torch.equal(m, a[1]) and mx == a[2] and gone == a[3]
    # remove, then insert the same ids into the clusters they came from: the restated update (they move behind the survivors)
    seg = np.repeat(np.arange(len(SIZES)), SIZES)
    in_index = np.isin(mem, ids)
    back = np.sort(mem[in_index])
    home = seg[in_index][np.argsort(mem[in_index])].astype(np.int32)
    o2, m2, mx2 = ops.cluster_insert(a[0], a[1], up(back), up(home))
    want_o, want_m = lifecycle_ref.update(offs, mem, back, home)
    assert np.array_equal(o2.cpu().numpy(), want_o) and np.array_equal(m2.cpu().numpy(), want_m)
    assert np.array_equal(want_o, offs) and mx2 == max(SIZES)


def test_device_index_remove_and_shrink_cluster_index(dev):
    from gdr_amd.modeling import shrink_cluster_index
    rng, offs, mem = _index(seed=29)
    names = ["0-%d" % c for c in range(len(SIZES))]
    idx = codec.ClusterIndex(names, offs, mem)
    rows = rng.choice(N_IDS, 2500, replace=True)                     # any order, with repeats
    want_o, want_m, want_n = lifecycle_ref.remove(offs, mem, rows)
    small = shrink_cluster_index(idx, rows, device=dev)
    assert small.names == names and np.array_equal(small.offsets, want_o) and np.array_equal(small.members, want_m)
    dci = ops.DeviceClusterIndex(idx, dev, 30, position=1, kary=30)
    old = dci.struct.members
    assert dci.remove(_up(dev)(np.unique(rows))) == want_n
    assert np.array_equal(dci.offsets.cpu().numpy(), want_o) and np.array_equal(dci.members[:dci.n_members].cpu().numpy(), want_m)
    assert dci.n_members == len(want_m) and dci.max_cluster == int(np.diff(want_o).max())
    assert dci.struct.members == dci.members.data_ptr() != old and dci.struct.offsets == dci.offsets.data_ptr()
    assert dci.remove(_up(dev)(mem[np.argsort(mem)])) == len(want_m)  # everything: the members array keeps one unused entry
    assert dci.n_members == 0 and dci.max_cluster == 0 and dci.members.numel() == 1


# ------------------------------------------------------------------------------------------------ the retriever
def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=GDRConfig.tiny().max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")


@pytest.fixture(scope="module")
def tiny_setup(dev):
    """The tiny model over V*V clusters of 3 documents, one batch of 4 queries and the step output of the index as built."""
    from gdr_amd.modeling import GDRModel, GDRRetriever
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
    base = GDRRetriever(model, torch.from_numpy(D0).to(dev), idx, _args(V)).validation_step_i(batch)
    cent, counts = expand_ref.centroids(D0, idx.offsets, idx.members)
    return types.SimpleNamespace(cfg=cfg, V=V, idx=idx, D0=D0, model=model, batch=batch, csz=csz, cent=cent, counts=counts,
                                 base_ids=base["doc_id_tensor"].cpu().numpy(), base_clusters=[list(r) for r in base["clusters"]])


def _same_step(a, b):
    return torch.equal(a["doc_id_tensor"].cpu(), b["doc_id_tensor"].cpu()) and torch.equal(a["rerank_values"].cpu(), b["rerank_values"].cpu())


def _retriever(s, dev, D=None, index=None, **kw):
    from gdr_amd.modeling import GDRRetriever
    return GDRRetriever(s.model, torch.from_numpy(s.D0 if D is None else D).to(dev), s.idx if index is None else index, _args(s.V), **kw)


def test_remove_documents_equals_fresh_retriever(dev, tiny_setup):
    """Fails without the feature.  Removed: the best document of every query, every member of one cluster that query 0 decodes
    (the cluster stays, empty, and is still decoded), and the first member of EVERY cluster, so that the largest cluster — and
    the candidate stride — shrinks from 3 to 2."""
    s = tiny_setup
    N0 = len(s.D0)
    top = s.base_ids[:, :, 0].reshape(-1)
    assert (top >= 0).all()
    whole = s.idx[s.base_clusters[0][0]]
    assert len(whole) == s.csz
    ids = np.concatenate([top, whole, np.arange(0, N0, s.csz), top])          # unsorted, with repeats
    want_o, want_m, want_n = lifecycle_ref.remove(s.idx.offsets, s.idx.members, ids)
    restated = s.idx.with_csr(want_o, want_m)
    ref = _retriever(s, dev, index=restated).validation_step_i(s.batch)
    outs = []
    for device_candidates in (True, False):
        r = _retriever(s, dev, device_candidates=device_candidates)
        r.validation_step_i(s.batch)                                         # the device index exists before the removal
        assert r.remove_documents(ids) == want_n
        assert np.array_equal(r.index.offsets, want_o) and np.array_equal(r.index.members, want_m)
        assert r.doc_embed.shape[0] == N0                                    # rows stay: doc ids never shift
        dci = r._device_index()
        assert (dci is not None) == device_candidates
        if dci is not None:
            assert dci.max_cluster == 2 and dci.n_members == len(want_m)
            assert np.array_equal(dci.members[:dci.n_members].cpu().numpy(), want_m)
        out = r.validation_step_i(s.batch)
        assert _same_step(out, ref), f"device_candidates={device_candidates}: not the step of a fresh retriever over the restated index"
        got = out["doc_id_tensor"].cpu().numpy()
        assert not np.isin(got, ids).any(), "a removed document is still retrieved"
        assert r.remove_documents(ids) == 0                                  # already gone: ignored
        assert np.array_equal(r.index.members, want_m)
        outs.append(got)
    assert (outs[0] >= 0).any() and not np.array_equal(outs[0], s.base_ids)


def _moves(s, n=12, seed=3):
    """n documents with new embeddings whose nearest centroid is clearly (fp64 gap above the fp32 band) another cluster's."""
    rng = np.random.default_rng(seed)
    N0 = len(s.D0)
    ids = rng.choice(N0, 60, replace=False)
    X = (s.D0[(ids + N0 // 2) % N0] * np.float32(1.5) + 1e-3 * rng.standard_normal((60, s.D0.shape[1]))).astype(np.float32)
    tgt, gap, band = expand_ref.assign(X, s.cent, s.counts)
    ok = (gap > 4 * band) & (tgt != ids // s.csz)
    assert ok.sum() >= n, "not enough documents whose nearest centroid changes"
    pick = np.nonzero(ok)[0][:n]
    return ids[pick], X[pick], tgt[pick]


def test_update_documents_equals_fresh_retriever(dev, tiny_setup):
    s = tiny_setup
    ids, X, tgt = _moves(s)                                                  # ids in random order
    want_o, want_m = lifecycle_ref.update(s.idx.offsets, s.idx.members, ids, tgt)
    D1 = s.D0.copy()
    D1[ids] = X
    ref = _retriever(s, dev, D=D1, index=s.idx.with_csr(want_o, want_m)).validation_step_i(s.batch)
    for device_candidates in (True, False):
        r = _retriever(s, dev, device_candidates=device_candidates)
        cl = r.update_documents(ids, torch.from_numpy(X).to(dev))
        assert cl.dtype == np.int32 and np.array_equal(cl, tgt)
        assert np.array_equal(r.index.offsets, want_o) and np.array_equal(r.index.members, want_m)
        assert np.array_equal(r.doc_embed.cpu().numpy().view(np.uint32), D1.view(np.uint32))
        assert _same_step(r.validation_step_i(s.batch), ref)
    # an id that was removed earlier is restored by an update, into the cluster of its nearest frozen centroid
    r = _retriever(s, dev)
    back, _gap, _band = expand_ref.assign(s.D0[ids], s.cent, s.counts)
    assert (_gap > _band).all()
    assert r.remove_documents(ids) == len(ids) and not np.isin(r.index.members, ids).any()
    assert np.array_equal(r.update_documents(ids[:5], torch.from_numpy(s.D0[ids[:5]]).to(dev)), back[:5])
    o1, m1, _ = lifecycle_ref.remove(s.idx.offsets, s.idx.members, ids)
    want = expand_ref.merge(o1, m1, ids[:5], back[:5])
    assert np.array_equal(r.index.offsets, want[0]) and np.array_equal(r.index.members, want[1])
    dci = r._device_index()
    assert np.array_equal(dci.members[:dci.n_members].cpu().numpy(), want[1])
    with pytest.raises(_ffi.GdrError, match="twice"):
        r.update_documents([3, 3], torch.from_numpy(s.D0[:2]).to(dev))
    assert np.array_equal(r.index.members, want[1])


def test_centroids_are_those_of_the_index_as_built(dev, tiny_setup):
    """Whichever of add / remove / update comes first, and whatever follows, the frozen centroids are the same bits."""
    s = tiny_setup
    ids, X, _tgt = _moves(s)
    want = s.cent.view(np.uint32)
    Xd = torch.from_numpy(X).to(dev)
    calls = {"add": lambda r: r.add_documents(Xd), "remove": lambda r: r.remove_documents(np.arange(0, 60)),
             "update": lambda r: r.update_documents(ids, Xd)}
    for first in calls:
        r = _retriever(s, dev)
        for name in [first] + [n for n in calls if n != first]:
            calls[name](r)
            assert np.array_equal(r._centroids.centroids.cpu().numpy().view(np.uint32), want), f"centroids moved after {name} (first: {first})"
        # clusters 0 .. 19 lost every member as built; a centroid that is kept can still receive documents
        assert (r._centroids.counts > 0).all()


def test_update_documents_overwrites_and_widens_tokens(dev):
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
    tok, msk = (torch.from_numpy(a).to(dev) for a in synth.make_tokens(5, L=32, vocab_hi=bc["vocab_size"], seed=6))
    r = GDRRetriever(None, D0.clone(), idx, _args(30), doc_tower=tower, doc_tokens=(tok0, msk0))
    ids = np.array([400, 7, 599, 0, 123])
    with pytest.raises(_ffi.GdrError, match="tokens"):
        r.update_documents(ids, embeds=D0[:5])
    with pytest.raises(_ffi.GdrError, match="token rows"):
        r.update_documents(ids[:4], embeds=D0[:4], tokens=(tok, msk))
    assert r.doc_tokens[0].shape == (N0, 24) and torch.equal(r.doc_embed, D0) and np.array_equal(r.index.members, idx.members)
    cl = r.update_documents(ids, tokens=(tok, msk))
    emb = tower(passage={"input_ids": tok, "attention_mask": msk})
    rows = torch.from_numpy(ids).to(dev)
    assert torch.equal(r.doc_embed[rows], emb)
    assert np.array_equal(cl, ops.FrozenCentroids(D0, idx).assign(emb).cpu().numpy())
    assert r.doc_tokens[0].shape == (N0, 32) and torch.equal(r.doc_tokens[0][rows], tok) and torch.equal(r.doc_tokens[1][rows], msk)
    keep = torch.ones(N0, dtype=torch.bool, device=dev)
    keep[rows] = False
    for new, old in zip(r.doc_tokens, (tok0, msk0)):
        assert torch.equal(new[keep][:, :24], old[keep]) and int(new[keep][:, 24:].abs().sum()) == 0
    assert torch.equal(r.doc_embed[keep], D0[keep])
    # a shorter passage: written into the same buffers, PAD 0 / mask 0 behind it
    p0 = r.doc_tokens[0].data_ptr()
    r.update_documents([7], tokens=(tok[:1, :20], msk[:1, :20]))
    assert r.doc_tokens[0].data_ptr() == p0 and torch.equal(r.doc_tokens[0][7, :20], tok[0, :20])
    assert int(r.doc_tokens[0][7, 20:].abs().sum()) == 0 and int(r.doc_tokens[1][7, 20:].abs().sum()) == 0
    # and add_documents still appends behind the widened table
    r.add_documents(tokens=(tok[:3], msk[:3]))
    assert r.doc_tokens[0].shape == (N0 + 3, 32) and torch.equal(r.doc_tokens[0][N0:], tok[:3])
    assert torch.equal(r.doc_tokens[0][rows[2:]], tok[2:])


def test_lifecycle_refusals_change_nothing(dev, tiny_setup):
    from gdr_amd.modeling import GDRRetriever
    s = tiny_setup
    D = torch.from_numpy(s.D0).to(dev)
    N0, d = s.D0.shape
    X = D[:2].clone()
    sh = GDRRetriever(None, D, s.idx, _args(s.V), sharded=types.SimpleNamespace(D=D))
    bf = GDRRetriever(None, D.to(torch.bfloat16), s.idx, _args(s.V))
    for r, word in ((sh, "sharded"), (bf, "bf16")):
        with pytest.raises(_ffi.GdrError, match=word):
            r.remove_documents([1, 2])
        with pytest.raises(_ffi.GdrError, match=word):
            r.update_documents([1, 2], X)
        assert r.index is s.idx and getattr(r, "_centroids", None) is None
    r = GDRRetriever(None, D.clone(), s.idx, _args(s.V))
    for bad in ([0, N0], [-1], [1.5]):
        with pytest.raises(_ffi.GdrError, match="doc ids|integers"):
            r.remove_documents(bad)
    with pytest.raises(_ffi.GdrError, match="doc ids"):
        r.update_documents([1, N0], X)
    with pytest.raises(_ffi.GdrError, match="embeds must be"):
        r.update_documents([1, 2], X[:, :d // 2].contiguous())
    with pytest.raises(_ffi.GdrError, match="2 ids but 1 embeddings"):
        r.update_documents([1, 2], X[:1])
    with pytest.raises(_ffi.GdrError, match="embeds= or tokens="):
        r.update_documents([1, 2])
    assert r.index is s.idx and torch.equal(r.doc_embed, D) and not hasattr(r, "_dci")
    assert r.remove_documents([]) == 0 and r.update_documents([], X[:0]).size == 0 and r.index is s.idx
