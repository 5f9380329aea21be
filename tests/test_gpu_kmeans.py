"""Hierarchical k-means docid construction on the MI355X: gdr_kmeans_assign / gdr_kmeans_partition through the C ABI
and gdr_amd.kmeans.build_docids against the reference's golden (g15) and the numpy restatement (tests/kmeans_ref.py); properties
of the tree; the refusals; the index end to end through GDRRetriever / add_documents and tools/build_index.py."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import batch_rounds as BR
import expand_ref
import kmeans_ref as kr
from conftest import REPO, golden
from gdr_amd import _ffi, codec, kmeans, ops, synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g15():
    return golden("g15_kmeans")


def _same_tree(out, digits, leaves):
    rd, rl = kr.pad_digits(digits)
    names, offs, mem = kr.cluster_csr(leaves)
    assert np.array_equal(out.lengths, rl), "id lengths differ"
    assert np.array_equal(out.digits, rd), "id digits differ"
    assert out.cluster_index.names == names, "cluster names differ"
    assert np.array_equal(out.cluster_index.offsets, offs) and np.array_equal(out.cluster_index.members, mem)


def test_lloyd_from_c0_equals_sklearn(dev, g15):
    """(b) one level from sklearn's C0: sklearn's labels exactly, its centres within the fp32 summation bound
    n_j * 2^-24 * max|x| per component."""
    g = g15
    X, k = g["X"], int(g["k"])
    D, C0 = torch.from_numpy(X).to(dev), torch.from_numpy(g["C0"].astype(np.float32)).to(dev)
    assert np.array_equal(g["C0"].astype(np.float32).astype(np.float64), g["C0"]), "C0 are fixture rows: exact in fp32"
    for T in g["T_list"]:
        out = kmeans.build_docids(D, k=k, c=X.shape[0], max_iter=int(T), init_centroids=C0, max_depth=2)
        lab = out.digits[:, 0]
        sk_lab, sk_cen = g[f"sk_labels_T{T}"], g[f"sk_centers_T{T}"]
        assert np.array_equal(lab, sk_lab), f"T={T}: {int((lab != sk_lab).sum())} labels differ from sklearn"
        # centres after T updates: the members of update T are the labels of the E-step before it; sklearn reports the same
        n_j = np.bincount(kr.lloyd(X.astype(np.float64), g["C0"], int(T) - 1)[0] if T > 1 else kr.assign(X.astype(np.float64), g["C0"])[0],
                          minlength=k)
        bound = n_j[:, None] * 2.0 ** -24 * float(np.abs(X).max())
        err = np.abs(out.root_centroids.astype(np.float64) - sk_cen)
        print(f"T={T}: max centre error {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
        assert (err <= bound).all()
        assert abs(out.inertia - float(g[f"sk_inertia_T{T}"])) <= 1e-4 * out.inertia


@pytest.mark.parametrize("which", ["n_init_1", "default"])
def test_whole_tree_equals_restatement(dev, g15, which):
    """(c) build_docids on the fixture = the float64 restatement's tree, exactly; the recipe asserted the margins that make the
    comparison meaningful (every score gap >= 4x the fp32 bound, competing restarts >= 1e-4 apart).  Fails without the feature."""
    g = g15
    X, k, c, seed = g["X"], int(g["k"]), int(g["c"]), int(g["seed"])
    n_init = 1 if which == "n_init_1" else kmeans.DEFAULT_N_INIT
    assert kmeans.DEFAULT_N_INIT == int(g["default_n_init"])
    stats = {}
    digits, leaves = kr.build(X, k, c, seed, int(g["max_iter"]), n_init, stats=stats)
    want = float(g["tree_inertia_n1"] if which == "n_init_1" else g["tree_inertia_default"])
    assert abs(stats["inertia"] - want) <= 1e-12 * want, "the restatement no longer builds the recipe's tree"
    out = kmeans.build_docids(torch.from_numpy(X).to(dev), k=k, c=c, seed=seed, max_iter=int(g["max_iter"]), n_init=n_init)
    _same_tree(out, digits, leaves)
    print(f"{which}: device inertia {out.inertia:.9g}, restatement {stats['inertia']:.9g}")
    assert abs(out.inertia - stats["inertia"]) <= 1e-4 * stats["inertia"]
    assert out.id_mapping()[0] == digits[0] and len(out.id_mapping()) == X.shape[0]


def test_two_builds_are_bit_identical(dev):
    X = synth.make_corpus(6000, 64, cluster_size=12, seed=4)
    D = torch.from_numpy(X).to(dev)
    a = kmeans.build_docids(D, k=8, c=8, n_init=2, max_depth=12)
    b = kmeans.build_docids(D, k=8, c=8, n_init=2, max_depth=12)
    assert np.array_equal(a.digits, b.digits) and np.array_equal(a.lengths, b.lengths) and a.inertia == b.inertia
    assert a.cluster_index.names == b.cluster_index.names and np.array_equal(a.cluster_index.members, b.cluster_index.members)
    assert np.array_equal(a.root_centroids.view(np.uint32), b.root_centroids.view(np.uint32))
    # properties: every leaf <= c docs, ids unique, cluster names prefix-free (Trie.from_docids), every doc in exactly one cluster
    idx = a.cluster_index
    assert np.diff(idx.offsets).max() <= 8 and np.diff(idx.offsets).min() >= 1
    assert np.array_equal(np.sort(idx.members), np.arange(6000))
    assert len(set(a.docid_strings())) == 6000
    names = set(idx.names)
    for n in idx.names:
        parts = n.split("-")
        assert all("-".join(parts[:i]) not in names for i in range(1, len(parts))), f"cluster {n} lies below another cluster"
    codec.Trie.from_docids(idx.names, 8)
    for cl in range(0, len(idx.names), 97):                    # a doc's id = its cluster's name (+ its rank in a leaf of >= 2)
        mem = idx.members[idx.offsets[cl]:idx.offsets[cl + 1]]
        for rank, m in enumerate(mem):
            want = idx.names[cl] + ("-%d" % rank if len(mem) > 1 else "")
            assert "-".join(str(x) for x in a.digits[m, :a.lengths[m]]) == want
    assert all(np.all(np.diff(idx.members[idx.offsets[i]:idx.offsets[i + 1]]) > 0) for i in range(len(idx.names)))


def test_a_node_alone_and_inside_a_level_gets_the_same_bits(dev):
    rng = np.random.default_rng(9)
    N, d, k = 9000, 768, 30
    X = synth.make_corpus(N, d, seed=6)
    D = torch.from_numpy(X).to(dev)
    sizes = [2500, 31, 900, 129, 3000, 64]
    perm = rng.permutation(N)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(perm[off[i]:off[i + 1]]) for i in range(len(sizes))]).astype(np.int32)
    cent = np.concatenate([X[rng.choice(rows[off[i]:off[i + 1]], k, replace=False)] for i in range(len(sizes))])
    lab, sc, ch, st = ops.kmeans_assign(D, torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(cent).to(dev), k)
    assert int(st.item()) == 0 and np.array_equal(ch.cpu().numpy(), sizes)
    for i in (1, 2, 4):
        r = torch.from_numpy(rows[off[i]:off[i + 1]].copy()).to(dev)
        o = torch.tensor([0, sizes[i]], dtype=torch.int32, device=dev)
        l1, s1, _c, _s = ops.kmeans_assign(D, r, o, torch.from_numpy(cent[i * k:(i + 1) * k].copy()).to(dev), k)
        assert torch.equal(l1, lab[off[i]:off[i + 1]])
        assert torch.equal(s1.view(torch.int32), sc[off[i]:off[i + 1]].view(torch.int32)), "score bits depend on the launch"
    # prev_labels: only the labels that differ are counted
    prev = lab.clone()
    prev[:7] = (prev[:7] + 1) % k
    _l, _s, ch2, _st = ops.kmeans_assign(D, torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(cent).to(dev), k,
                                         prev_labels=prev)
    assert ch2.cpu().tolist() == [7, 0, 0, 0, 0, 0]


def test_partition_is_a_stable_counting_sort(dev):
    rng = np.random.default_rng(2)
    # batch_rounds.PARTITION_CASES: part_scan_kernel at 1024, 1025 and 1023 scan entries (one per thread, two, and an idle last thread)
    for k, sizes in ((30, [70000, 1, 255, 256, 257, 31, 5000]), (64, [3, 1000]), (2, [513])) + BR.PARTITION_CASES:
        n = sum(sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        rows = np.concatenate([np.sort(rng.choice(10 ** 6, s, replace=False)) for s in sizes]).astype(np.int32)
        lab = rng.integers(0, k, n).astype(np.int32)
        lab[off[-2]:off[-1]][::2] = k - 1
        crow, coff, st = ops.kmeans_partition(torch.from_numpy(rows).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(off).to(dev), k)
        assert int(st.item()) == 0
        er, eo = [], [0]
        for i in range(len(sizes)):
            r, l = rows[off[i]:off[i + 1]], lab[off[i]:off[i + 1]]
            for j in range(k):
                er.append(r[l == j])
                eo.append(eo[-1] + len(er[-1]))
        assert np.array_equal(coff.cpu().numpy(), np.array(eo, np.int32))
        assert np.array_equal(crow.cpu().numpy(), np.concatenate(er))
    bad = torch.from_numpy(lab).to(dev).clone()
    bad[5] = k
    _r, _o, st = ops.kmeans_partition(torch.from_numpy(rows).to(dev), bad, torch.from_numpy(off).to(dev), k)
    assert int(st.item()) & 1, "a label outside [0, k) must be reported"


def test_update_is_the_fixed_shape_two_stage_sum(dev):
    """gdr_kmeans_centroids: bit-identical to the numpy restatement (chunks of 256 from the child's start, chunk sums in order);
    a child of <= 256 members has gdr_cluster_centroids' bits; an empty child has count 0 and a zero row."""
    rng = np.random.default_rng(8)
    N, d = 6000, 96
    X = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float32)
    sizes = [1000, 0, 3, 256, 257, 600, 1, 0, 513, 255, 2048, 0]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(rng.choice(N, s, replace=False)) for s in sizes]).astype(np.int32)
    D = torch.from_numpy(X).to(dev)
    cent, counts = ops.kmeans_centroids(D, torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev))
    cent2, _ = ops.kmeans_centroids(D, torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev))
    assert torch.equal(cent.view(torch.int32), cent2.view(torch.int32))
    assert counts.cpu().tolist() == sizes
    cent = cent.cpu().numpy()
    seq, _n = ops.cluster_centroids_csr(D, torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev))
    seq = seq.cpu().numpy()
    for c, sz in enumerate(sizes):
        if sz == 0:
            assert not cent[c].any()
            continue
        want = kr.two_stage_mean(X, rows[off[c]:off[c + 1]])
        assert np.array_equal(cent[c].view(np.uint32), want.view(np.uint32)), f"child {c} ({sz} members)"
        if sz <= 256:
            assert np.array_equal(cent[c].view(np.uint32), seq[c].view(np.uint32))
    # d = 768 (three column slices), a child that starts in the middle of a slot and spans several
    X7 = synth.make_corpus(3000, 768, seed=3)
    off7 = np.array([0, 100, 100, 1500, 3000], np.int32)
    c7, n7 = ops.kmeans_centroids(torch.from_numpy(X7).to(dev), torch.from_numpy(off7).to(dev), torch.arange(3000, dtype=torch.int32, device=dev))
    for c in (0, 2, 3):
        want = kr.two_stage_mean(X7, np.arange(off7[c], off7[c + 1]))
        assert np.array_equal(c7[c].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert n7.cpu().tolist() == [100, 0, 1400, 1500] and not c7[1].any().item()


def test_identical_rows_terminate_by_the_degenerate_rule(dev):
    X = np.tile(np.random.default_rng(1).standard_normal(16).astype(np.float32), (100, 1))
    out = kmeans.build_docids(torch.from_numpy(X).to(dev), k=4, c=6, n_init=2, max_depth=6)
    digits, leaves = kr.build(X, 4, 6, n_init=2)
    _same_tree(out, digits, leaves)
    assert len(set(out.docid_strings())) == 100 and np.diff(out.cluster_index.offsets).max() <= 6


def test_an_emptied_child_keeps_its_centroid_and_is_absent(dev):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((400, 32)).astype(np.float32)
    C0 = np.concatenate([X[:5], 100.0 * np.ones((1, 32), np.float32)])            # centroid 5: |c|^2 / 2 = 160,000 — never the argmax
    out = kmeans.build_docids(torch.from_numpy(X).to(dev), k=6, c=400, init_centroids=torch.from_numpy(C0).to(dev), max_depth=2)
    assert (out.digits[:, 0] != 5).all() and set(out.cluster_index.names) == {"0", "1", "2", "3", "4"}
    assert np.array_equal(out.root_centroids[5].view(np.uint32), C0[5].view(np.uint32)), "the emptied child's centroid moved"
    assert np.isfinite(out.root_centroids).all() and not np.array_equal(out.root_centroids[:5], C0[:5])


def test_refusals(dev):
    X = torch.from_numpy(synth.make_corpus(300, 32, seed=2)).to(dev)
    with pytest.raises(_ffi.GdrError, match="bf16"):
        kmeans.build_docids(X.to(torch.bfloat16))
    with pytest.raises(_ffi.GdrError, match="d=30"):
        kmeans.build_docids(X[:, :30].contiguous())
    with pytest.raises(_ffi.GdrError, match="d=4100"):
        kmeans.build_docids(torch.zeros((8, 4100), device=dev))
    for k in (1, 65):
        with pytest.raises(_ffi.GdrError, match=f"k={k}"):
            kmeans.build_docids(X, k=k)
    with pytest.raises(_ffi.GdrError, match="output_vocab_size=10"):
        kmeans.build_docids(X, k=4, c=12, kary=10)
    with pytest.raises(_ffi.GdrError, match="output_vocab_size=6"):
        kmeans.build_docids(X, k=8, c=4, kary=30, output_vocab_size=6)
    with pytest.raises(_ffi.GdrError, match="CUDA"):
        kmeans.build_docids(X.cpu())
    with pytest.raises(_ffi.GdrError, match=r"of \d+ docs at depth \d+ needs ids longer than max_depth=2"):
        kmeans.build_docids(X, k=2, c=2, n_init=1, max_depth=2)
    with pytest.raises(_ffi.GdrError, match="init_centroids"):
        kmeans.build_docids(X, k=4, init_centroids=X[:3])
    with pytest.raises(_ffi.GdrError, match="bf16"):
        ops.kmeans_assign(X.to(torch.bfloat16), torch.arange(300, dtype=torch.int32, device=dev),
                          torch.tensor([0, 300], dtype=torch.int32, device=dev), X[:4], 4)
    with pytest.raises(_ffi.GdrError, match="int32"):
        ops.kmeans_partition(torch.arange(300, device=dev), torch.zeros(300, dtype=torch.int32, device=dev),
                             torch.tensor([0, 300], dtype=torch.int32, device=dev), 4)


def test_every_row_of_a_768_wide_round_is_within_the_fp32_band(dev):
    """(d) d = 768, k = 30, N = 20,000, one root round from init_centroids: for EVERY row the float64 score of the label the
    device chose lies within (2d + 8) * 2^-24 * |x| * max|c| of that row's float64 maximum.  No row is excluded."""
    N, d, k = 20000, 768, 30
    X = synth.make_corpus(N, d, seed=11)
    C0 = X[np.random.default_rng(5).choice(N, k, replace=False)]
    D = torch.from_numpy(X).to(dev)
    lab, sc, ch, st = ops.kmeans_assign(D, torch.arange(N, dtype=torch.int32, device=dev), torch.tensor([0, N], dtype=torch.int32, device=dev),
                                        torch.from_numpy(C0).to(dev), k)
    lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
    assert int(st.item()) == 0 and int(ch.item()) == N and lab.min() >= 0 and lab.max() < k
    X64, C64 = X.astype(np.float64), C0.astype(np.float64)
    s = X64 @ C64.T - 0.5 * (C64 * C64).sum(1)[None, :]
    band = (2 * d + 8) * 2.0 ** -24 * np.linalg.norm(X64, axis=1) * np.linalg.norm(C64, axis=1).max()
    chosen = s[np.arange(N), lab]
    deficit = s.max(1) - chosen
    print(f"labels that differ from the float64 argmax: {np.mean(lab != s.argmax(1)):.5%}; largest deficit / band "
          f"{(deficit / band).max():.3e}; largest |device score - float64 score| / band {(np.abs(sc - chosen) / band).max():.3e}")
    assert (deficit <= band).all(), f"{int((deficit > band).sum())} rows chose a centroid outside the fp32 band"
    assert (np.abs(sc - chosen) <= band).all()
    # the same round inside build_docids gives the same labels
    out = kmeans.build_docids(D, k=k, c=N, max_iter=1, init_centroids=torch.from_numpy(C0).to(dev), max_depth=2)
    assert out.levels[0]["rounds"] == 1


def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=GDRConfig.tiny().max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_end_to_end_retrieval_and_expansion_over_a_built_index(dev, tmp_path):
    """(e) build_docids -> GDRRetriever over that index -> validation_steps; add_documents on top gives the CSR expand_ref
    predicts; tools/build_index.py writes a clusters.npz that loads back equal."""
    from gdr_amd.modeling import GDRModel, GDRRetriever
    cfg = GDRConfig.tiny()
    V = cfg.output_vocab_size
    sd = synth.make_state_dict(cfg, seed=1234)
    N0 = 72
    D0 = synth.make_corpus(N0, cfg.d_model, cluster_size=6, seed=8) * np.float32(0.05)
    depth = kmeans.max_depth_for(cfg.max_output_length)
    assert depth == 3
    built = kmeans.build_docids(torch.from_numpy(D0).to(dev), k=V, c=V, max_depth=depth, kary=V, output_vocab_size=V)
    idx = built.cluster_index
    assert all(b is not None and len(b) <= depth for b in idx.token_bodies(V, 1, V))
    trie = codec.Trie.from_docids(idx.names, V)
    model = GDRModel(cfg, sd, dev, trie=trie, prefix_trie=trie)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    batch = {"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)}
    r = GDRRetriever(model, torch.from_numpy(D0).to(dev), idx, _args(V))
    outs = list(r.validation_steps([batch, batch]))
    assert len(outs) == 2
    for o in outs:
        got = o["doc_id_tensor"].cpu().numpy()
        assert got.shape[0] == 4 and got.max() < N0
        for b in range(4):                                     # every returned document is a member of a decoded cluster
            cand = {m for name in o["clusters"][b] for m in idx[name]}
            assert cand, "the trie-constrained decode must land on clusters of the built index"
            assert {int(x) for x in got[b].reshape(-1) if x >= 0} <= cand
    # expansion on top of the built index
    rng = np.random.default_rng(4)
    new = (D0[rng.integers(0, N0, 40)] + 1e-3 * rng.standard_normal((40, cfg.d_model)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    cent, counts = expand_ref.centroids(D0, idx.offsets, idx.members)
    tgt, gap, band = expand_ref.assign(new, cent, counts)
    assert (gap > 4 * band).all(), "the test's own inserted rows must not be near-ties"
    eo, em = expand_ref.merge(idx.offsets, idx.members, np.arange(N0, N0 + 40), tgt)
    new_ids, cl = r.add_documents(torch.from_numpy(new).to(dev))
    assert np.array_equal(np.asarray(cl), tgt) and np.array_equal(r.index.offsets, eo) and np.array_equal(r.index.members, em)
    assert r.index.names == idx.names
    r.validation_step_i(batch)
    # the CLI
    np.save(tmp_path / "emb.npy", D0)
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "build_index.py"), "--embeddings", str(tmp_path / "emb.npy"),
                        "--k", str(V), "--c", str(V), "--kary", str(V), "--max_output_length", str(cfg.max_output_length),
                        "--out", str(tmp_path / "clusters.npz"), "--idmapping", str(tmp_path / "ids.npz")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(tmp_path / "clusters.npz")
    back = codec.ClusterIndex([str(x) for x in z["cluster_names"]], z["cluster_offsets"], z["cluster_members"])
    assert back.names == idx.names and np.array_equal(back.offsets, idx.offsets) and np.array_equal(back.members, idx.members)
    zi = np.load(tmp_path / "ids.npz")
    assert np.array_equal(zi["digits"], built.digits) and np.array_equal(zi["lengths"], built.lengths)
