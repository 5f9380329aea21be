"""Cases, CPU-side builders and references of the batches that need more than one round of a one-workgroup "plan" kernel:
pack_scan_kernel (csrc/layers.hip: seq_off[] and the live-row count of every packed forward), rows_units_kernel (csrc/sim_rows.hip:
counts, status and the unit list of the gather top-k) and prefix_plan_kernel (csrc/decode.hip: the hit / miss compaction of the beam
rows).  Their prefix sums are csrc/scan.h's block scan, ROUND = 1024 threads wide: the first two in its round form (one round per 1024
entries, a carry between the rounds; rows_units_kernel is that loop written out), the third in its single-shot form (every thread sums
ceil(rows / 1024) consecutive rows first) — as are insert_scan_kernel's (csrc/cluster_insert.hip, section 4) and part_scan_kernel's
(csrc/kmeans.hip, section 5).  tests/test_batch_rounds_host.py checks on the CPU that every case reaches what it names;
tests/test_gpu_batch_rounds.py (and, for section 5, tests/test_gpu_kmeans.py) runs the cases on the GPU.  No test lives here.

Every bound below either names the existing test it was taken from (`source`) or carries the figure it was measured from and the
margin (`measured`, `margin`) — never a kernel's output.
"""
import functools
import types

import numpy as np
import torch

import gather_ref
import live_ref
import peaked
from gdr_amd import codec, synth
from gdr_amd.config import GDRConfig

ROUND = 1024                      # entries per round of the three plan kernels (their workgroup size)
GEMM_TILE_ROWS = 128              # token rows per GEMM tile in the packing rules
MIN_PACKED_TILES = 192            # encoder.hip ragged_packs / bert.hip bert_ragged_impl: fewer tiles run the padded form


# ==================================================================================================== 1. pack plan: the two towers
TOWER_L = 24
TOWER_BATCHES = (1023, 1024, 1025, 2049)        # one partial round, exactly one, two, three (pooled-only fp32 T5: 1024 + 1025)
TOWER_LONG = (1025, 130)                        # (B, L): the key-block attention of attention_long.hip reads seq_off past round one
T5_SEED, BERT_SEED, TOKEN_SEED = 401, 402, 403

# sequence -> mask pattern on either side of every round boundary; the last sequence of a batch gets length 2 afterwards
BOUNDARY_PATTERNS = {1022: "one", 1023: "full", 1024: "zero", 1025: "hole", 2046: "hole", 2047: "one", 2048: "full"}
LAST_LEN = 2


def t5_config():
    return GDRConfig.tiny(**peaked.CFG64)       # d_model 128, d_kv 64, 4 heads, d_ff 256, 2 layers


@functools.lru_cache(maxsize=None)
def t5_state_dict():
    return synth.make_state_dict(t5_config(), seed=T5_SEED, with_decoder=False)


def bert_cfg():
    return synth.bert_config(tiny=True)         # hidden 128, 2 heads of 64, d_ff 256, 2 layers


@functools.lru_cache(maxsize=None)
def bert_state_dict():
    return synth.make_bert_state_dict(bert_cfg(), seed=BERT_SEED)


def gemm_tiles(B, L, d_model):
    return -(-(B * L) // GEMM_TILE_ROWS) * -(-d_model // GEMM_TILE_ROWS)


def t5_packs(cfg, B, L):
    """encoder.hip ragged_packs: the un-split packed forms."""
    return (cfg.d_kv == 64 and gemm_tiles(B, L, cfg.d_model) >= MIN_PACKED_TILES and cfg.d_model % 32 == 0 and cfg.d_ff % 32 == 0
            and (cfg.num_heads * cfg.d_kv) % 32 == 0)


def t5_packs_small(cfg, B, L):
    """encoder.hip ragged_packs_small: the split-K / stream-K forms over the live rows (fp32 only), where ragged_packs says no."""
    return cfg.d_kv == 64 and B * L >= 256 and cfg.d_model % 32 == 0 and cfg.d_ff % 32 == 0 and (cfg.num_heads * cfg.d_kv) % 32 == 0


def t5_chains(cfg, B, L):
    """Batches of the packed forwards, each with a pack plan of its own, that a pooled-only fp32 call runs (encoder.hip
    enc_chains_eligible, GDR_ENC_CHAINS at its default): the halves [0, B/2) and [B/2, B) where the smaller one still packs."""
    if B >= 2 and cfg.num_layers >= 2 and t5_packs(cfg, B // 2, L):
        return (B // 2, B - B // 2)
    return (B,)


def bert_packs(bc, B, L):
    """bert.hip bert_ragged_impl: `packs && tiles >= 192` (fp32; the bf16 and split forms exist only packed and need d, d_ff % 128)."""
    d, H, dff = bc["hidden_size"], bc["num_heads"], bc["d_ff"]
    return d % H == 0 and d // H == 64 and d % 128 == 0 and dff % 128 == 0 and gemm_tiles(B, L, d) >= MIN_PACKED_TILES


def rounds(n):
    return -(-n // ROUND)


def tower_shapes():
    return [(B, TOWER_L) for B in TOWER_BATCHES] + [TOWER_LONG]


@functools.lru_cache(maxsize=None)
def tower_tokens(B, L, vocab):
    """(ids, mask) int64 [B, L]: synth.make_tokens(min_len = 1) with the sequences around every round boundary set to
    BOUNDARY_PATTERNS and the last sequence to LAST_LEN tokens.  Read-only: shared by every test of a shape."""
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=vocab, seed=TOKEN_SEED + B + L, min_len=1)
    g = np.random.Generator(np.random.PCG64(TOKEN_SEED * 7 + B))

    def prefix(b, n):
        ids[b] = g.integers(2, vocab, size=L)
        mask[b] = np.arange(L) < n
        ids[b, n - 1] = 1
        ids[b] *= mask[b]

    for b, pattern in BOUNDARY_PATTERNS.items():
        if b >= B:
            continue
        if pattern == "one":
            prefix(b, 1)
        elif pattern == "full":
            prefix(b, L)
        else:                                           # not right padding: the sequence keeps every position and its mask
            ids[b] = g.integers(2, vocab, size=L)
            mask[b] = 0 if pattern == "zero" else 1
            if pattern == "hole":
                mask[b, L // 3:L // 2] = 0
    prefix(B - 1, LAST_LEN)
    ids.setflags(write=False)
    mask.setflags(write=False)
    return ids, mask


def kept(mask):
    """Rows the packed form computes (include/gdr_hip.h): the leading ones of a non-empty prefix mask, else the whole sequence."""
    m = np.asarray(mask) != 0
    B, L = m.shape
    n = m.sum(1)
    is_prefix = (n > 0) & (m == (np.arange(L)[None, :] < n[:, None])).all(1)
    return np.where(is_prefix[:, None], m, True)


def sample_sequences(B):
    """The sequences held against the CPU oracle: both sides of every round boundary, the first and the last."""
    return sorted({s for s in (0, 1022, 1023, 1024, 1025, 2047, 2048, B - 1) if 0 <= s < B})


def _with_fp32_mask_rows(run, sd, mask):
    """The float64 oracle of the rows, except where a mask is all zeros: the reference adds (1 - m) * -1e9 to the scores IN FP32,
    where -1e9 (ulp 64) absorbs every score and the softmax is exactly uniform — the kernels' answer too.  A float64 sum keeps the
    scores beside -1e9 and attends as if the mask were all ones, which is another model.  Those rows take the fp32 oracle."""
    out = run(peaked.as_float64(sd), slice(None)).numpy().copy()
    zero = np.nonzero(np.asarray(mask).sum(1) == 0)[0]
    if zero.size:
        out[zero] = run(sd, zero).double().numpy()
    return out


def t5_oracle(ids, mask, bf16=False, f64=True):
    """Hidden states float64 [n, L, d] of oracle/t5_ref.py on the given sequences (see _with_fp32_mask_rows)."""
    from oracle import t5_ref
    cfg, ti, tm = t5_config(), torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(mask))

    def run(sd, rows):
        if bf16:
            with t5_ref.bf16_linears():
                return t5_ref.encoder_forward(sd, cfg, ti[rows], tm[rows])
        return t5_ref.encoder_forward(sd, cfg, ti[rows], tm[rows])

    if not f64:
        return run(t5_state_dict(), slice(None)).double().numpy()
    return _with_fp32_mask_rows(run, t5_state_dict(), mask)


def bert_oracle(ids, mask, bf16=False, f64=True):
    """Hidden states float64 [n, L, d] of oracle/bert_ref.py on the given sequences (see _with_fp32_mask_rows)."""
    from oracle import bert_ref
    bc, ti, tm = bert_cfg(), torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(mask))

    def run(sd, rows):
        return bert_ref.bert_forward(sd, bc, ti[rows], tm[rows], bf16=bf16)[0]

    if not f64:
        return run(bert_state_dict(), slice(None)).double().numpy()
    return _with_fp32_mask_rows(run, bert_state_dict(), mask)


@functools.lru_cache(maxsize=None)
def tower_sample(tower, B, L, bf16=False, f64=True):
    """(sample sequence numbers, their ids, mask, kept rows, oracle hidden states) of a tower shape; computed once, read-only."""
    vocab = t5_config().vocab_size if tower == "t5" else bert_cfg()["vocab_size"]
    ids, mask = tower_tokens(B, L, vocab)
    rows = sample_sequences(B)
    si, sm = ids[rows], mask[rows]
    ref = (t5_oracle if tower == "t5" else bert_oracle)(si, sm, bf16=bf16, f64=f64)
    ref.setflags(write=False)
    return rows, si, sm, kept(sm), ref


def bf16_noise(tower, B, L):
    """|emulation with fp32 sums - emulation with float64 sums| over the kept rows of the sample sequences whose mask is not all zeros
    (those rows have one reference, _with_fp32_mask_rows): (max, mean)."""
    _, _, sm, keep, e64 = tower_sample(tower, B, L, True, True)
    e32 = tower_sample(tower, B, L, True, False)[4]
    keep = keep & (sm.sum(1) > 0)[:, None]
    d = np.abs(e32 - e64)[keep]
    return float(d.max()), float(d.mean())


# form -> how its output is held.  `exact`: bit for bit against the padded form of the same handle, which never touches the pack plan.
# Otherwise `bound` (absolute and relative) against the float64 oracle on sample_sequences, and `vs_fp32`: the cap on max |pooled -
# pooled of the fp32 packed form| over EVERY sequence, where an existing test states one for the form.
_PARITY = "tests/test_gpu_parity.py::test_encoder_split_bf16_form_vs_reference_golden_and_the_fp32_form"
_T5_LONG = "tests/test_gpu_t5_long.py::test_long_encoder_split_forms_vs_fp32_path"
_DOC_SPLIT = "tests/test_gpu_decode.py::test_doc_tower_split_form_keeps_fp32_level_embeddings"
# bert-bf16: no test runs the bf16 doc tower on un-scaled synthesised weights at these widths (test_gpu_peaked.py scales q by 6),
# so the noise was measured here: bf16_noise("bert", B, 24) = (max, mean) at B = 1023, 1024, 1025, 2049:
# (7.3e-7, 1.1e-7), (6.8e-7, 1.1e-7), (5.27e-3, 5.24e-4), (6.13e-3, 4.57e-4).  The noise is one discrete event: an activation that
# rounds to the other bf16 neighbour under the other summation order moves its row by a few 1e-3 through the LayerNorms that follow.
# The two or three sequences sampled at B <= 1024 happen to hold no such flip, the six and eight sampled above do; whether two correct
# implementations flip in a given handful of rows is chance, so every shape is held to the largest figures over the four shapes
# (the eight-sequence sample), x 4 as in tests/peaked.py
BERT_BF16_NOISE = (6.13e-3, 5.24e-4)
TOWER_FORMS = {
    "t5-fp32": dict(tower="t5", kw={}, exact=True, source="tests/test_gpu_ragged.py::test_ragged_rows_bit_identical_to_padded_form"),
    "t5-bf16": dict(tower="t5", kw=dict(dtype=torch.bfloat16), exact=True,
                    source="tests/test_gpu_ragged.py::test_ragged_bf16_mode_bit_identical_to_padded_bf16"),
    # the three split forms are held to the fp32 path's own 2e-4 against the reference golden; pooled against the fp32 form: 1e-4
    # (six terms), 5e-5 (fp16 x 2) at d_model 128 / d_kv 64 / d_ff 256, 2e-4 (three terms: 16 bits carried)
    "t5-split6": dict(tower="t5", kw=dict(split=6), exact=False, bound=2e-4, source=_PARITY, vs_fp32=1e-4, vs_fp32_source=_T5_LONG),
    "t5-split3": dict(tower="t5", kw=dict(split=3), exact=False, bound=2e-4, source=_PARITY, vs_fp32=2e-4, vs_fp32_source=_PARITY),
    "t5-split2": dict(tower="t5", kw=dict(split=2), exact=False, bound=2e-4, source=_PARITY, vs_fp32=5e-5, vs_fp32_source=_T5_LONG),
    "bert-fp32": dict(tower="bert", kw={}, exact=True,
                      source="tests/test_gpu_decode.py::test_doc_tower_ragged_form_is_bit_identical_to_the_padded_form"),
    # bert_config(tiny=True) through the split form against the reference golden: 1e-4; pooled within 5e-5 of the fp32 packed form
    "bert-split": dict(tower="bert", kw=dict(split=True), exact=False, bound=1e-4, source=_DOC_SPLIT, vs_fp32=5e-5,
                       vs_fp32_source=_DOC_SPLIT),
    "bert-bf16": dict(tower="bert", kw=dict(dtype=torch.bfloat16), exact=False, bf16=True, measured=BERT_BF16_NOISE, margin=4.0),
}


# ==================================================================================================== 2. gather top-k
GATHER_N, GATHER_D, GATHER_K, GATHER_CAP = 5000, 64, 10, 4096
GATHER_BATCHES = (1024, 1025, 2050)
GATHER_SLICE = 512                # rule (a): a slice of at most this many queries stays inside one round of rows_units_kernel
GATHER_TOL = 1e-4                 # tests/test_gpu_query_gather.py TOL (oracle/parity_rules.py)
ROWS_UNIT = 16                    # csrc/sim_rows.hip ROWS_UNIT: allowed rows per unit of the flat unit list
# (B, bf16 corpus) -> query seed: the first from 1 on that leaves no sampled query with a reference tie at its cut (chosen on the CPU
# by scan_gather_seeds; test_batch_rounds_host.py asserts it)
GATHER_QSEED = {(1024, False): 1, (1024, True): 1, (1025, False): 1, (1025, True): 1, (2050, False): 1, (2050, True): 2}


def gather_samples(B):
    return sorted({q for q in (0, 1023, 1024, 1025, 2047, 2048, B - 1) if 0 <= q < B})


def gather_designed_counts(B):
    """query -> allowed rows, for the queries set by hand (the last query's 33 rows are set last)."""
    want = {1023: 0, 1024: 1, 1025: 17, 2047: GATHER_N, 2048: 0}
    want = {q: c for q, c in want.items() if q < B}
    want[B - 1] = 33
    return want


@functools.lru_cache(maxsize=None)
def gather_allowed(B):
    """bool [B, N]: a random density between 0.2 % and 5 % per query, then the queries of gather_designed_counts."""
    rng = np.random.default_rng(9000 + B)
    a = rng.random((B, GATHER_N)) < rng.uniform(0.002, 0.05, size=(B, 1))
    for q, c in gather_designed_counts(B).items():
        a[q] = False
        if c == 1:
            a[q, GATHER_N - 1] = True                   # the last row: the last bit of the last bitmap word in use
        elif c == GATHER_N:
            a[q] = True
        elif c:
            a[q, rng.choice(GATHER_N, size=c, replace=False)] = True
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gather_corpus():
    D = synth.make_corpus(GATHER_N, GATHER_D, seed=GATHER_N + GATHER_D)
    D.setflags(write=False)
    return D


def _gather_case(B, bf16, seed):
    D = gather_corpus()
    Q, _ = synth.make_queries(D, B, seed=seed)
    Qt, Dt = torch.from_numpy(Q), torch.from_numpy(np.array(D))
    if bf16:
        Qt, Dt = Qt.bfloat16(), Dt.bfloat16()
    sample = gather_samples(B)
    S = live_ref.scores(Qt[sample].double().numpy(), Dt.double().numpy())      # the operands as the kernel sees them
    return types.SimpleNamespace(B=B, N=GATHER_N, d=GATHER_D, k=GATHER_K, bf16=bf16, Qt=Qt, Dt=Dt, allowed=gather_allowed(B),
                                 sample=sample, S=S)


@functools.lru_cache(maxsize=None)
def gather_case(B, bf16):
    """Operands (torch, CPU), bitmaps, the sampled queries and their fp64 scores [len(sample), N]; made once, never modified."""
    return _gather_case(B, bf16, GATHER_QSEED[(B, bf16)])


def gap_ok(scores, rows, k, tol=GATHER_TOL):
    """The k-th and (k + 1)-th best scores over `rows` are further apart than the parity rule's tie width."""
    v = np.sort(scores[rows])[::-1]
    return v.size <= k or bool(v[k - 1] - v[k] > 2 * tol * (1 + abs(v[k - 1])))


def gather_cut_ties(s, cap):
    """The sampled queries whose reference has a tie at the cut of the top-k over their first `cap` allowed rows."""
    bad = []
    for j, q in enumerate(s.sample):
        rows, _ = gather_ref.rows_of(live_ref.pack(s.allowed[q]), s.N, cap)
        if not gap_ok(s.S[j], rows, s.k):
            bad.append(q)
    return bad


def scan_gather_seeds(B, bf16, seeds):
    """Yields (seed, sampled queries with a tie at a cut — of the gather list and of the dense list over every allowed row)."""
    for seed in seeds:
        s = _gather_case(B, bf16, seed)
        yield seed, sorted(set(gather_cut_ties(s, GATHER_CAP)) | set(gather_cut_ties(s, 2 ** 20)))


def check_topk_rows(S, allowed, queries, vals, ids, k, cap, what, tol=GATHER_TOL):
    """The rule tests/test_gpu_query_gather.py applies (its _check, strict): S fp64 [len(queries), N]; vals / ids numpy rows of those
    queries.  A short list ends in -inf / -1, every id is one of the query's ranked rows, the reference has no tie at the cut, values
    within tol, ids exact outside the reference's tolerance-tie groups."""
    from oracle.parity_rules import order_insensitive_topk_match
    N = S.shape[1]
    rv, ri, _ = gather_ref.topk(S, allowed[queries], k, cap)
    for j, q in enumerate(queries):
        rows, _ = gather_ref.rows_of(live_ref.pack(allowed[q]), N, cap)
        c = int(min(rows.size, k))
        assert (ids[j, c:] == -1).all() and np.isneginf(vals[j, c:]).all(), f"{what}: query {q}: the tail of a short list is -inf / -1"
        got = ids[j, :c].astype(np.int64)
        assert np.isin(got, rows).all(), f"{what}: query {q} was given a row outside its ranked rows"
        assert gap_ok(S[j], rows, k, tol), f"{what}: query {q}: the reference has a tie at the cut; choose another seed"
        order_insensitive_topk_match(rv[j:j + 1, :c], ri[j:j + 1, :c], vals[j:j + 1, :c], got[None], tol)


# ==================================================================================================== 3. prefix-table decode
PREFIX_R = 6
PREFIX_L = 9
PREFIX_TOL = 1e-4                 # peaked.fp32_bound's floor, the tolerance of tests/test_gpu_prefix.py against the oracle
PREFIX_MAX_EXCUSED = 0.02
PREFIX_SD_SEED = 1234
# B -> (beam rows, rows per thread, threads that own a row)
PREFIX_BATCHES = {350: (2100, 3, 700), 171: (1026, 2, 513)}
PREFIX_KEEP_EVERY = (3, 7)
# B -> token seed: the first from 1 on whose float64 search leaves at most 2 % of the beam rows inside the tie window (chosen on the
# CPU by scan_prefix_seeds; test_batch_rounds_host.py asserts it)
PREFIX_TOKEN_SEED = {350: 1, 171: 1}


def prefix_config():
    return GDRConfig.tiny()


@functools.lru_cache(maxsize=None)
def prefix_state_dict():
    return synth.make_state_dict(prefix_config(), seed=PREFIX_SD_SEED)


def tiny_docids(V, depth, keep_every=1):
    """As tests/test_gpu_prefix.py builds them: every keep_every-th docid of the full V ** depth space."""
    return ["-".join(str(x) for x in synth.cluster_digits(c, depth, V)) for c in range(V ** depth) if c % keep_every == 0]


def prefix_trie(keep_every):
    V = prefix_config().output_vocab_size
    return codec.Trie.from_docids(tiny_docids(V, 2, keep_every), V)


def prefix_tokens(B, seed=None):
    cfg = prefix_config()
    return synth.make_tokens(B, L=PREFIX_L, vocab_hi=cfg.vocab_size, seed=PREFIX_TOKEN_SEED[B] if seed is None else seed, min_len=2)


def _prefix_oracle(B, seed):
    from oracle import beam_ref, t5_ref
    cfg, R = prefix_config(), PREFIX_R
    sd = peaked.as_float64(prefix_state_dict())
    ids, mask = prefix_tokens(B, seed)
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask)).index_select(0, idx)
    mask_x = torch.from_numpy(mask).index_select(0, idx)
    trace, ptrace = [], []
    dec, sc = beam_ref.beam_search(lambda seq: t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True), B, R,
                                   cfg.decode_vocab_size, cfg.max_output_length, 0.8, R, trace=trace, prefix_trace=ptrace)
    return peaked.hypothesis_lists(dec.numpy(), B, R), np.array(sc, np.float64).reshape(B, R), trace, ptrace


@functools.lru_cache(maxsize=None)
def prefix_oracle(B):
    """The search of oracle/beam_ref.generate(..., restricted_head=True) — the encoder once, its states expanded per beam, the
    restricted head — in float64, with the traces generate() does not hand out: (hypothesis lists per query, scores [B, R], trace,
    prefix_trace).  The beams are not constrained, so it does not depend on the trie."""
    return _prefix_oracle(B, PREFIX_TOKEN_SEED[B])


def scan_prefix_seeds(B, seeds):
    for seed in seeds:
        yield seed, peaked.tied_row_share(_prefix_oracle(B, seed)[1], PREFIX_TOL)


def prefix_hits(trie, prefixes):
    """bool [rows]: whether a beam row's token prefix (START, then tokens depth * V + c + 2) is a node of the trie."""
    V, hit = trie.V, np.zeros(len(prefixes), bool)
    for r, row in enumerate(np.asarray(prefixes).tolist()):
        node = 0
        for depth, tok in enumerate(row[1:]):
            c = tok - 2 - depth * V
            node = int(trie.child[node, c]) if 0 <= c < V and depth < 2 else -1
            if node < 0:
                break
        hit[r] = node >= 0
    return hit


def prefix_mixed_threads(B, keep_every):
    """Per later step (one whose beams can have left the trie) of the oracle's search: (step, threads of prefix_plan_kernel whose
    `per` consecutive rows hold both a hit and a miss, hit rows, miss rows)."""
    rows, per, _ = PREFIX_BATCHES[B]
    trie, ptrace = prefix_trie(keep_every), prefix_oracle(B)[3]
    out = []
    for s in range(2, len(ptrace)):
        hit = prefix_hits(trie, ptrace[s])
        assert hit.size == rows
        pad = np.zeros(-(-rows // per) * per, bool)
        any_hit, any_miss = pad.copy(), pad.copy()
        any_hit[:rows], any_miss[:rows] = hit, ~hit
        mixed = any_hit.reshape(-1, per).any(1) & any_miss.reshape(-1, per).any(1)
        out.append((s, int(mixed.sum()), int(hit.sum()), int((~hit).sum())))
    return out


# ==================================================================================================== 4. cluster insert
INSERT_C, INSERT_NEW = 2049, 500          # insert_scan_kernel: per = ceil(C / 1024) = 3, the last threads own no cluster


@functools.lru_cache(maxsize=None)
def insert_case():
    """(offsets int32 [C + 1], members int32 [n_old], new ids int32 [500] ascending, their clusters int32 [500]): random old sizes
    0 .. 6 with the clusters on either side of the thread boundaries 1023 | 1024 and 2046 .. 2048 set by hand."""
    rng = np.random.default_rng(77)
    sizes = rng.integers(0, 7, INSERT_C)
    sizes[[0, 1023, 2047]] = 0
    sizes[[1022, 1024, 2046, 2048]] = [5, 1, 3, 2]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n_old = int(offsets[-1])
    members = rng.permutation(n_old).astype(np.int32)
    new_ids = np.arange(n_old, n_old + INSERT_NEW, dtype=np.int32)
    targets = rng.integers(0, INSERT_C, INSERT_NEW).astype(np.int32)
    targets[:8] = [1023, 1024, 1024, 2047, 2048, 2048, 0, 1022]
    return offsets, members, new_ids, targets


REMOVE_EMPTIED = (1022, 1024, 2046, 2048)  # clusters that lose every member: on either side of the thread boundaries of per = 3


@functools.lru_cache(maxsize=None)
def remove_case():
    """(offsets, members, ids int32 strictly ascending) over insert_case's CSR — the removal mode of insert_scan_kernel (a negative
    histogram) at the same C = 2049: every member of the REMOVE_EMPTIED clusters, 400 members drawn at random, and one id that is a
    member of no cluster."""
    offsets, members, _, _ = insert_case()
    rng = np.random.default_rng(78)
    gone = [members[offsets[c]:offsets[c + 1]] for c in REMOVE_EMPTIED]
    ids = np.unique(np.concatenate(gone + [rng.choice(members, 400, replace=False), [members.size + 7]])).astype(np.int32)
    return offsets, members, ids


# ==================================================================================================== 5. k-means partition
KP_TILE = 256                              # csrc/kmeans.hip KP_TILE: rows of one partition work item
# (k, node sizes): part_scan_kernel scans m = k * (tiles of 256 rows over the nodes) counts, per = ceil(m / 1024) consecutive ones per
# thread: m = 1024 (one entry per thread), 1025 (per = 2, threads 0 .. 512 own entries), 1023 (the last thread owns none)
PARTITION_CASES = ((64, (4096,)), (41, (6400,)), (33, (256,) * 31))


def partition_scan_entries(k, sizes):
    return k * sum(-(-s // KP_TILE) for s in sizes)


if __name__ == "__main__":
    # from the repository root, with PYTHONPATH=.:tests :   python tests/batch_rounds.py   prints what the tables above record
    torch.set_grad_enabled(False)
    for B in TOWER_BATCHES:
        print(f"bert-bf16 noise B={B} L={TOWER_L}: max {bf16_noise('bert', B, TOWER_L)[0]:.3e} mean {bf16_noise('bert', B, TOWER_L)[1]:.3e}", flush=True)
    for B in GATHER_BATCHES:
        for bf16 in (False, True):
            print(f"gather B={B} bf16={bf16}:", [(seed, bad) for seed, bad in scan_gather_seeds(B, bf16, range(1, 6))], flush=True)
    for B in PREFIX_BATCHES:
        print(f"prefix B={B}:", [(seed, f"{100 * t:.2f} %") for seed, t in scan_prefix_seeds(B, range(1, 4))], flush=True)
        for ke in PREFIX_KEEP_EVERY:
            print(f"  keep_every={ke}: (step, mixed threads, hits, misses)", prefix_mixed_threads(B, ke), flush=True)
