"""The reference's Python call surface for the inference hot path, backed by libgdr_hip.so.

Drop-in targets:
  * `GDRModel.generate(...)`           T5ForConditionalGeneration.generate as GDR calls it
                                       (GDR_model/main_models.py:1380-1397, main.py:171-187;
                                        transformers/generation_utils.py:110-527)
  * `GDRModel.get_encoder()(...)`      transformers/modeling_t5.py:1319-1320, generation_utils.py:410-411
  * `QueryEncoder` / `EncoderModel`    GDR_model/main_models.py:79-109 (forward(query_enc=h) -> h[:,0])
  * `DenseModel`                       GDR_model/dense.py:30-54 (encode_query / encode_passage / compute_similarity)
  * `GDRRetriever.validation_step_i`   the two-stage retrieval of main_models.py:1337-1642 (decode -> rerank)
There is no CPU path: every method needs CUDA (ROCm) tensors and raises if the HIP library is missing.
"""
import types

import torch

from . import _ffi, codec, ops
from .config import GDRConfig, stage2_query_form


class ModelOutput(dict):
    """Minimal stand-in for transformers' BaseModelOutput: attribute + item access (file_utils.py ModelOutput)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def strip_lightning_prefix(state_dict, prefix="model."):
    """A Lightning checkpoint's `state_dict` prefixes T5 keys with `model.` and the doc tower with `encoder.`
    (main_models.py:794,797; main.py:121-126).  Returns the T5 part with the prefix removed."""
    if "state_dict" in state_dict:
        state_dict = state_dict["state_dict"]
    if any(k.startswith(prefix + "shared.") or k.startswith(prefix + "encoder.block") for k in state_dict):
        return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    return state_dict


class _Encoder:
    """What `model.get_encoder()` returns: callable like T5Stack.forward (modeling_t5.py:685-821)."""

    def __init__(self, handle):
        self.handle = handle

    def __call__(self, input_ids=None, attention_mask=None, return_dict=True, **_ignored):
        h, _ = self.handle.forward(input_ids, attention_mask, want_pooled=False)
        if return_dict:
            return ModelOutput(last_hidden_state=h, past_key_values=None, hidden_states=None, attentions=None)
        return (h,)

    forward = __call__


class GDRModel:
    """T5ForConditionalGeneration of the reference (GDR config: decode_embedding=2, adaptor_efficient — or, with
    GDRConfig(adaptor_decode=0, adaptor_efficient=0), the adaptor-free model whose docid head is the plain lm_head),
    inference only.  Construct from a reference-style state_dict (SURVEY Appendix C key names)."""

    def __init__(self, cfg: GDRConfig, state_dict, device="cuda:0", with_decoder=True, trie=None, ragged=False,
                 prefix_trie=None, dtype=torch.float32, graph=False):
        """trie: optional codec.Trie — enables the NCI trie constraint of the reference's earlier
        generation_utils_previous.py:714-729 (the shipped generate() ignores `decode_tree`).
        ragged: generate() skips the PAD rows of the encoder (gdr_t5_encoder_forward_ragged).  Decoded ids, scores and the
        CLS rows are unchanged (cross-attention masks PAD keys, kept rows are bit-identical); only the PAD positions of the
        `last_hidden_state` returned with output_encoder_embedding=True are zero instead of the reference's values there,
        hence opt-in.  get_encoder() always computes every row.
        prefix_trie: optional codec.Trie over the corpus' docids — builds the device prefix table (ops.PrefixTable) at
        load: beams whose prefix is a node of that trie read the query-independent adaptor/head results from it instead of
        recomputing them (modeling_t5.py:1618-1639); other beams are computed as before.  Same logits up to fp32
        summation order.  When `trie` (the constraint) is given too it must be the same trie.  Refused (GdrError) for an
        adaptor-free config (cfg.has_adaptor False: the head is lm_head alone, there is nothing to tabulate); trie= works there.
        dtype=torch.bfloat16: BASELINE config C5's precision mode (the reference has none: precision=32) — every linear of
        encoder, decoder, adaptor and head takes bf16 operands with fp32 accumulate; all other arithmetic stays fp32.
        graph: replay the decode (gdr_t5_generate) of a repeated call shape as one captured HIP graph instead of ~1 400
        host launches per call (ops.T5DecoderHandle.generate); same kernels, same results."""
        self.config = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.GdrError("GDRModel needs a CUDA (ROCm) device; there is no CPU path")
        if prefix_trie is not None and not cfg.has_adaptor:       # before any weight is moved to the device
            raise _ffi.GdrError("prefix_trie= needs the adaptor head: the prefix table stores the adaptor's query-independent "
                                "results, and an adaptor-free model (adaptor_decode=0, adaptor_efficient=0) has none — pass "
                                "trie= for the constraint alone")
        sd = strip_lightning_prefix(state_dict)
        self.dtype = dtype
        self.enc = ops.T5EncoderHandle(cfg, sd, self.device, dtype=dtype)
        self.dec = ops.T5DecoderHandle(cfg, sd, self.device, dtype=dtype) if with_decoder else None
        self.prefix_table = None
        if prefix_trie is not None:
            if self.dec is None:
                raise _ffi.GdrError("prefix_trie needs the decoder (with_decoder=True)")
            if trie is not None and trie is not prefix_trie:
                raise _ffi.GdrError("trie= and prefix_trie= must be the same codec.Trie object")
            self.prefix_table = ops.PrefixTable(self.dec, prefix_trie, self.device)
        if trie is None:
            self.trie = None
        else:                                     # the constraint shares the table's breadth-first arrays
            self.trie = self.prefix_table.device_trie if self.prefix_table is not None else ops.DeviceTrie(trie, self.device)
        self.graph = bool(graph)
        self.ragged = bool(ragged)
        self.training = False

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def get_encoder(self):
        return _Encoder(self.enc)

    # ------------------------------------------------------------------ generate()
    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, max_length=None, num_beams=None, length_penalty=None,
                 num_return_sequences=None, early_stopping=False, use_cache=False, do_sample=False,
                 decode_embedding=None, decode_vocab_size=None, output_scores=False, output_encoder_embedding=False,
                 **model_kwargs):
        """Same kwargs / return shape as the vendored generate(): returns `(output, encoder_outputs | None)` where
        output is `(LongTensor[B*nret, <=max_length], list[float])` with output_scores=True, else the LongTensor
        (generation_utils.py:524-527, 918-921).  num_beams=1 (the reference's default) is its greedy branch
        (_generate_no_beam_search, :553-627): output is the bare LongTensor[B, width] also with output_scores=True, width =
        the length at which the last row emitted EOS (or max_length).  Unknown kwargs (decode_tree, decoder_index, cluster_constraint,
        decoder_attention_mask, ...) are accepted and ignored exactly as the reference swallows them
        (modeling_t5.py:1755)."""
        cfg = self.config
        if self.dec is None:
            raise _ffi.GdrError("this GDRModel was built with with_decoder=False")
        assert input_ids is not None, "generate() needs input_ids"
        max_length = max_length if max_length is not None else cfg.max_output_length
        num_beams = num_beams if num_beams is not None else 1
        length_penalty = length_penalty if length_penalty is not None else 1.0
        num_return_sequences = num_return_sequences if num_return_sequences is not None else 1
        # the reference's asserts (generation_utils.py:296-324) for the arguments this path uses
        assert isinstance(max_length, int) and max_length > 0, "`max_length` should be a strictly positive integer."
        assert isinstance(num_beams, int) and num_beams > 0, "`num_beams` should be a strictly positive integer."
        assert length_penalty > 0, "`length_penalty` should be strictly positive."
        assert isinstance(num_return_sequences, int) and num_return_sequences > 0, \
            "`num_return_sequences` should be a strictly positive integer."
        if do_sample:
            raise NotImplementedError("sampling is outside the GDR hot path (gen_method='greedy', main.py:299)")
        if num_beams == 1:
            # no_beam_search greedy generation conditions (generation_utils.py:341-346)
            assert num_return_sequences == 1, \
                "Greedy decoding will always produce the same output for num_beams == 1 and num_return_sequences > 1. " \
                "Please set num_return_sequences = 1"
        assert num_return_sequences <= num_beams, "num_return_sequences has to be <= num_beams for greedy beam search"
        if decode_vocab_size is not None:
            assert decode_vocab_size == cfg.decode_vocab_size, "decode_vocab_size does not match the loaded head"
        assert 1 < max_length, "The context has 1 number of tokens, but `max_length` is only %d" % max_length
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        enc_h, ids, lens, scores = self._generate_launch(input_ids, attention_mask, num_beams, max_length, length_penalty,
                                                          num_return_sequences)
        if num_beams == 1:
            # _generate_no_beam_search returns input_ids alone (generation_utils.py:627): no scores, whatever output_scores says
            output = ops.finish_greedy_output(ids, lens)
        else:
            decoded, score_list = ops.finish_generate_output(ids, lens, scores, max_length)
            output = (decoded, score_list) if output_scores else decoded
        if output_encoder_embedding:
            # the reference hands back the states already expanded per beam (generation_utils.py:459-461);
            # callers stride them with [::num_beams] (main_models.py:1466)
            expanded = enc_h.repeat_interleave(num_beams, dim=0)
            return output, ModelOutput(last_hidden_state=expanded)
        return output, None

    @torch.no_grad()
    def score_docids(self, input_ids, docid_ids, attention_mask=None, length_penalty=1.0, hidden=False):
        """Teacher forcing: encodes the queries and runs the decoder over the GIVEN docid token rows instead of searching for them
        (ops.T5DecoderHandle.score).  docid_ids int64[B*n, width] holds n rows per query, query-major, each START, the docid's
        tokens, EOS, then PAD — what generate() returns at num_return_sequences == num_beams, gold docids or another system's
        candidates (codec encodes docid strings); width <= max_output_length.  Returns float64[B*n] on the device: each row's
        sum of token log-probabilities / len ** length_penalty, the score generate() reports for that hypothesis.  hidden=True
        returns (scores, trace, eos_state, mean) as ops.T5DecoderHandle.score does."""
        if self.dec is None:
            raise _ffi.GdrError("this GDRModel was built with with_decoder=False")
        assert input_ids is not None and docid_ids is not None, "score_docids() needs input_ids and docid_ids"
        assert length_penalty > 0, "`length_penalty` should be strictly positive."
        B = input_ids.shape[0]
        if docid_ids.dim() != 2 or docid_ids.shape[0] == 0 or docid_ids.shape[0] % B:
            raise ValueError(f"score_docids: docid_ids must hold a whole number of rows per query ({B} queries), got "
                             f"{tuple(docid_ids.shape)}")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        input_ids, attention_mask = input_ids.to(self.device), attention_mask.to(self.device)
        enc_h, _ = self.enc.forward(input_ids, attention_mask, want_pooled=False, ragged=self.ragged)
        return self.dec.score(enc_h, attention_mask, docid_ids.to(self.device, torch.int64), docid_ids.shape[0] // B,
                              length_penalty, hidden=hidden)

    def _generate_launch(self, input_ids, attention_mask, num_beams, max_length, length_penalty, num_return_sequences):
        """The device part of generate(): encoder + beam decode enqueued on the current stream, nothing read back.
        Returns (encoder states [B,L,d], ids, lens, scores) — device tensors that ops.finish_generate_output turns into
        what generate() returns."""
        input_ids, attention_mask = input_ids.to(self.device), attention_mask.to(self.device)
        enc_h, _ = self.enc.forward(input_ids, attention_mask, want_pooled=False, ragged=self.ragged)
        ids, lens, scores = self.dec.generate(enc_h, attention_mask, num_beams, max_length, length_penalty,
                                              num_return_sequences, trie=self.trie, prefix_table=self.prefix_table,
                                              graph=self.graph)
        return enc_h, ids, lens, scores


class EncoderModel:
    """main_models.py:62-109.  `encoder(query_enc=hidden) -> hidden[:, 0]` (CLS pool; `output` is None in the reference);
    `encoder(passage={'input_ids','attention_mask'[, 'token_type_ids']}) -> pooler_output` of the DPR/BERT doc tower
    (modeling_dpr.py:146-191) when built with `bert=` (an ops.BertEncoderHandle)."""

    def __init__(self, output=None, bert=None, ragged=False):
        self.output, self.bert, self.ragged = output, bert, ragged

    @staticmethod
    def from_state_dict(bcfg, state_dict, device, prefix="ctx_encoder.bert_model.", dtype=torch.float32, ragged=None, split=False):
        """state_dict with the reference's doc-tower keys; a Lightning checkpoint prefixes them `encoder.model.`.
        ragged: PAD positions of a padded batch are not computed (bit-identical pooled output in fp32; r06).  dtype=torch.bfloat16:
        the bf16 precision mode (bf16 linear operands, fp32 accumulate), which exists in the ragged form only."""
        sd = state_dict.get("state_dict", state_dict)
        lp = "encoder.model."
        if any(k.startswith(lp) for k in sd):
            sd = {k[len(lp):]: v for k, v in sd.items() if k.startswith(lp)}
        ragged = (dtype == torch.bfloat16 or bool(split)) if ragged is None else ragged
        return EncoderModel(bert=ops.BertEncoderHandle(bcfg, sd, device, prefix, dtype=dtype, split=split), ragged=ragged)

    def __call__(self, passage=None, query_enc=None):
        if passage is not None:
            if self.bert is None:
                raise _ffi.GdrError("EncoderModel was built without doc-tower weights (use EncoderModel.from_state_dict)")
            p = {k: v.view(-1, v.size(-1)) for k, v in passage.items()}              # main_models.py:81-82
            _, pooled = self.bert.forward(p["input_ids"], p.get("attention_mask"), p.get("token_type_ids"),
                                          want_hidden=False, ragged=self.ragged)
            return pooled
        return self.encode_query(query_enc)

    def encode_passage(self, psg):
        return None if psg is None else self(passage=psg)

    forward = __call__

    def encode_query(self, qry_hidden):
        if qry_hidden is None:
            return None
        return qry_hidden[:, 0] if self.output is None else self.output(q=qry_hidden)


class DensePooler:
    """dense.py:10-27: rep = Linear(h[:,0]) (+ L2 normalise)."""

    def __init__(self, weight_q, bias_q, weight_p=None, bias_p=None, normalize=False):
        self.wq, self.bq = weight_q, bias_q
        self.wp, self.bp = (weight_p if weight_p is not None else weight_q), (bias_p if bias_p is not None else bias_q)
        self.normalize = normalize

    def __call__(self, q=None, p=None):
        if q is not None:
            rep = ops.linear(q[:, 0].contiguous(), self.wq, epilogue=_ffi.EPI_BIAS, bias=self.bq)
        elif p is not None:
            rep = ops.linear(p[:, 0].contiguous(), self.wp, epilogue=_ffi.EPI_BIAS, bias=self.bp)
        else:
            raise ValueError
        if self.normalize:
            rep = ops.l2_normalize(rep)
        return rep


class DenseModel:
    """dense.py:30-54 bi-encoder contract over two callables returning `.last_hidden_state`."""

    def __init__(self, lm_q, lm_p=None, pooler=None):
        self.lm_q, self.lm_p, self.pooler = lm_q, (lm_p if lm_p is not None else lm_q), pooler
        self._ws = None

    def encode_passage(self, psg):
        if psg is None:
            return None
        h = self.lm_p(**psg, return_dict=True).last_hidden_state
        return self.pooler(p=h) if self.pooler is not None else h[:, 0]

    def encode_query(self, qry):
        if qry is None:
            return None
        h = self.lm_q(**qry, return_dict=True).last_hidden_state
        return self.pooler(q=h) if self.pooler is not None else h[:, 0]

    def compute_similarity(self, q_reps, p_reps):
        """scores = q_reps @ p_reps.T (dense.py:53-54) — materialises [B,N]; prefer search() for top-k."""
        return ops.linear(q_reps.contiguous(), p_reps.contiguous())

    def __call__(self, query=None, passage=None):
        """EncoderModel.forward, eval branch (encoder.py:77-113): EncoderOutput(q_reps, p_reps[, scores], loss=None)."""
        q_reps, p_reps = self.encode_query(query), self.encode_passage(passage)
        if q_reps is None or p_reps is None:
            return ModelOutput(q_reps=q_reps, p_reps=p_reps, loss=None, scores=None)
        return ModelOutput(loss=None, scores=self.compute_similarity(q_reps, p_reps), q_reps=q_reps, p_reps=p_reps)

    forward = __call__

    def search(self, q_reps, p_reps, k, live=None, allowed=None, gather=None):
        """compute_similarity + topk(k) fused (never writes the score matrix). Returns (values, int64 indices).
        live: an ops.LiveRows over the rows of p_reps — rank its live rows only (k <= live.count); ids stay row numbers.
        allowed: an ops.QueryRows — a row filter per query (ANDed with live); a query with fewer than k allowed rows ends in -inf / -1.
        gather: ops.sim_topk's, for a call with allowed=: None (default) routes by the filters' row counts ("auto": queries that allow
        at most ops.GATHER_MAX_ROWS rows are scored over those rows only), False is the dense masked call, an int forces the gather mode.
        p_reps: the passage embeddings [N,d] (fp32, or bf16 = the C5 precision mode), or an ops.PrefilteredCorpus built from them once
        (the same fp32 top-k through the bf16 pre-filter, gdr_sim_topk_prefilter).  1 <= k <= min(ops.SIM_TOPK_MAX_K, N); past
        ops.PREFILTER_MAX_K a PrefilteredCorpus is searched on the plain fp32 path (the same list)."""
        if self._ws is None:
            self._ws = ops.Workspace(q_reps.device)
        v, i = ops.sim_topk(q_reps.contiguous(), p_reps, k, workspace=self._ws, exact_on_overflow=True, live=live, allowed=allowed,
                            gather="auto" if gather is None and allowed is not None else gather)
        return v, i.to(torch.int64)


class LazyRows:
    """A list that is built on first use.  GDRRetriever's step output names clusters and docs as STRINGS, as the reference's
    does (main_models.py:1398,1629-1633) — at 512 queries x 7 alphas x 10 docs that is 40 000 Python strings per step, several
    milliseconds of host time that a caller who only consumes `rerank_values` / the id tensors (or a benchmark loop) never
    needs.  Behaves like the list it stands for: len, indexing, iteration, == with a list or another LazyRows."""

    def __init__(self, n, make):
        self._n, self._make, self._val = n, make, None

    def _get(self):
        if self._val is None:
            self._val = self._make()
            self._make = None
        return self._val

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())

    def __eq__(self, other):
        return self._get() == (other._get() if isinstance(other, LazyRows) else other)

    def __ne__(self, other):
        return not self.__eq__(other)

    def __repr__(self):
        return repr(self._get())


def expand_cluster_index(doc_embed, index, rows, centroids=None):
    """Inserts the documents `rows` (ascending doc ids, rows of doc_embed fp32[N,d] on the GPU that belong to no cluster) into
    the cluster with the nearest centroid — the reference's tree_embedding_insert (main_models.py:268-295, run at :877-889
    over every row >= --docnum).  centroids: an ops.FrozenCentroids (default: computed from `index` as it stands).
    Returns (the expanded codec.ClusterIndex, names unchanged; the cluster index of every inserted row, int32 numpy)."""
    import numpy as np
    if doc_embed.dtype != torch.float32:
        raise _ffi.GdrError("corpus expansion needs the fp32 corpus (the bf16 precision mode is not supported)")
    fc = centroids if centroids is not None else ops.FrozenCentroids(doc_embed, index)
    dev = doc_embed.device
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size and (np.any(np.diff(rows) <= 0) or rows[0] < 0 or rows[-1] >= doc_embed.shape[0]):
        raise _ffi.GdrError("expand_cluster_index: rows must be ascending doc ids of the corpus")
    ids = torch.from_numpy(rows.astype(np.int32)).to(dev)
    tgt = fc.assign(doc_embed.index_select(0, ids.long()) if rows.size else doc_embed[:0], compact=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    offs, mem, _mx = ops.cluster_insert(up(index.offsets), up(index.members), ids, tgt, fc.cmap)
    csr = torch.cat([offs, mem]).cpu().numpy()                                      # one read-back of the merged CSR
    C_ = len(index.names)
    return index.with_csr(csr[:C_ + 1], csr[C_ + 1:]), fc.cmap[tgt.long()].cpu().numpy()


def shrink_cluster_index(index, rows, device=None):
    """The counterpart of expand_cluster_index: takes the documents `rows` (doc ids, any order, repeats allowed) out of the
    clusters of `index` (codec.ClusterIndex) through the device call (ops.cluster_remove) — every cluster keeps its other
    members in their order, a row that is in no cluster is ignored, names unchanged.  Returns the shrunk codec.ClusterIndex."""
    import numpy as np
    dev = torch.device(device if device is not None else "cuda")
    rows = np.asarray(rows).reshape(-1)
    if rows.size and (not np.issubdtype(rows.dtype, np.integer) or rows.min() < 0 or rows.max() >= 2 ** 31):
        raise _ffi.GdrError("shrink_cluster_index: rows must be int32 doc ids")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    offs, mem, _mx, _gone = ops.cluster_remove(up(index.offsets), up(index.members), up(np.unique(rows)))
    csr = torch.cat([offs, mem]).cpu().numpy()                                      # one read-back of the compacted CSR
    C_ = len(index.names)
    return index.with_csr(csr[:C_ + 1], csr[C_ + 1:])


class GDRRetriever:
    """Two-stage GDR retrieval = `T5FineTuner.validation_step_i` (main_models.py:1337-1642):
    beam-decode cluster ids -> id_mapping lookup -> tanh(q·d) over the candidates -> + alpha*softmax(beam scores)
    per cluster -> top-k, for every alpha in score_rate."""

    @staticmethod
    def _need_beams(args):
        if getattr(args, "num_return_sequences", None) == 1:
            raise _ffi.GdrError("GDRRetriever needs num_return_sequences >= 2: with one sequence generate() takes the greedy branch, "
                                "which returns no scores for validation_step_i to unpack (main_models.py:1400)")

    def __init__(self, model: GDRModel, doc_embed, cluster_index: codec.ClusterIndex, args, doc_tower=None,
                 doc_tokens=None, device_candidates=True, sharded=None, search_prefilter=False):
        """doc_embed: fp32 (or, in the C5 precision mode, bf16) [N, d] resident on the GPU (the reference's `self.doc_embed`).
        doc_tower + doc_tokens=(input_ids int64[N,Lp], attention_mask) enable the stage-2 re-encode path of
        main_models.py:1445-1455 (`epoch > train_encoder_epoch`): candidate docs are embedded on the fly by the
        BERT/DPR tower instead of being looked up (tokenisation itself is out of scope: tokens come pre-computed).
        sharded: a dist.ShardedIndex — BASELINE config C5's layout of this path (SURVEY §8e "for GDR mode, whole clusters"):
        the corpus is row-sharded over the ranks of one node (`doc_embed` may then be None: the rank's rows are
        `sharded.D`), every rank encodes and beam-decodes ITS OWN queries (generate() is data-parallel, as the reference's
        per-GPU launch is: Data_process/NQ_dataset/bert/bert_NQ.sh:5-12), and stage 2 is `sharded.rerank_own` — one
        all-gather of the queries + candidate blocks, per-shard scoring, one all-to-all, merge: the lists are bit-identical
        to the unsharded rerank.  Every rank must call validation_step_i the same number of times with the same batch size
        (the collectives are fixed-size); `cluster_index` is the index of the WHOLE corpus on every rank.
        search_prefilter: True = search() goes through the bf16 pre-filter over the live rows (ops.PrefilteredCorpus(doc_embed,
        masks=True), built on the first search: +50 % of doc_embed's memory; the same documents, values the same dot products in
        another summation order) and add_documents / update_documents keep the image current.  Needs the fp32 doc_embed of an
        unsharded retriever (GdrError otherwise).  The default leaves search() what it was."""
        self._need_beams(args)
        # the stage-2 query vector: the encoder CLS row, or per hypothesis the decoder's EOS state / masked mean
        self.query_form, why = stage2_query_form(args, sharded=sharded is not None)
        if why:
            raise _ffi.GdrError("GDRRetriever: " + why)
        self.model, self.args, self.index = model, args, cluster_index
        self.doc_embed = doc_embed if doc_embed is not None or sharded is None else sharded.D
        self.sharded = sharded
        if sharded is not None and not device_candidates:
            raise _ffi.GdrError("GDRRetriever(sharded=...) exchanges the device candidate blocks: device_candidates must stay on")
        self.encoder = doc_tower if doc_tower is not None else EncoderModel()
        self.doc_tokens = doc_tokens
        # device_candidates: decoded rows -> clusters -> candidate CSR on the GPU (gdr_cluster_candidates); False keeps the
        # host form (decode_token strings + ClusterIndex.candidates) — same lists, one D2H / H2D round trip more per step
        self.device_candidates = bool(device_candidates)
        self.search_prefilter = bool(search_prefilter)
        if self.search_prefilter:
            if sharded is not None:
                raise _ffi.GdrError("GDRRetriever(search_prefilter=True): a sharded retriever has no dense search() to pre-filter")
            if self.doc_embed is None or self.doc_embed.dtype != torch.float32:
                raise _ffi.GdrError("GDRRetriever(search_prefilter=True) needs the fp32 doc_embed (a bf16 corpus is its own image)")

    @property
    def live_rows(self):
        """ops.LiveRows over doc_embed: a row is live iff it is a member of some cluster.  Built on first use from the member CSR
        and kept current by add_documents / remove_documents / update_documents.  A sharded retriever has none."""
        if self.sharded is not None:
            raise _ffi.GdrError("live_rows: a sharded retriever keeps no live-row mask (sharded removal is not supported)")
        if getattr(self, "_live", None) is None:
            import numpy as np
            N = self.doc_embed.shape[0]
            mem = np.asarray(self.index.members, dtype=np.int64).reshape(-1)
            live = np.zeros(N, dtype=bool)
            live[mem[(mem >= 0) & (mem < N)]] = True
            self._live = ops.LiveRows.from_bool(torch.from_numpy(live).to(self.doc_embed.device))
        return self._live

    @torch.no_grad()
    def search(self, q_reps, k, allowed=None, gather=None):
        """The dense top-k of q_reps [B, d] over the LIVE documents (DenseModel.search with live_rows): a document withdrawn by
        remove_documents never comes back, one restored by update_documents does, ids are rows of doc_embed.  Returns (values,
        int64 ids); k <= the number of live documents.  allowed: an ops.QueryRows over doc_embed's rows — a filter per query, ANDed
        with live_rows (a removed document never returns, whatever the filter says); a query left with fewer than k documents ends
        in -inf / -1.  gather: as DenseModel.search's (None routes narrow filters to the gather mode).  Raises GdrError for a sharded retriever."""
        live = self.live_rows
        if getattr(self, "_search_ws", None) is None:
            self._search_ws = ops.Workspace(self.doc_embed.device)
        corpus = self.doc_embed
        if self.search_prefilter:                                    # the image is made here, once, and kept current from then on
            if getattr(self, "_prefiltered", None) is None:
                self._prefiltered = ops.PrefilteredCorpus(self.doc_embed, masks=True)
            corpus = self._prefiltered
        v, i = ops.sim_topk(q_reps.contiguous(), corpus, k, workspace=self._search_ws, live=live, allowed=allowed,
                            gather="auto" if gather is None and allowed is not None else gather)
        return v, i.to(torch.int64)

    @torch.no_grad()
    def add_documents(self, embeds=None, tokens=None):
        """Adds n documents to the corpus without retraining the generative model (the GDR paper's scalability claim; the
        reference's tree_embedding_insert, main_models.py:268-295): each joins the cluster whose centroid has the largest fp32
        dot product with it (ties: the lower cluster index).  embeds: fp32 [n, d]; or tokens=(input_ids int64[n, Lp],
        attention_mask) — pre-tokenised passages that the retriever's doc tower (doc_tower=) embeds.  With the re-encode path
        configured (doc_tokens=), tokens= is required and appended to doc_tokens.
        The rows are appended to doc_embed (backing buffer grown geometrically) and become doc ids N .. N+n-1.  The centroids
        are frozen on the first call from the index as built and never updated, as in the reference: adding in k calls gives
        the index that one call gives.  The merged CSR replaces both the device index and the host ClusterIndex (one read-back),
        so the device_candidates=False / --kary 0 paths see the same lists.  Returns (doc ids int64[n], cluster indices int32[n]
        into cluster_index.names).
        Must not run while validation_steps() has steps in flight: their candidate lists and doc_embed would change under them.
        Raises GdrError for a sharded retriever, a bf16 doc_embed (the C5 precision mode) and a dimension mismatch."""
        import numpy as np
        if self.sharded is not None:
            raise _ffi.GdrError("add_documents: a sharded retriever cannot take documents (sharded insertion is not supported)")
        if self.doc_embed is None or self.doc_embed.dtype != torch.float32:
            raise _ffi.GdrError("add_documents needs the fp32 doc_embed (the bf16 precision mode is not supported)")
        dev = self.doc_embed.device
        N, d = self.doc_embed.shape
        embeds, tok, msk = self._document_rows("add_documents", embeds, tokens)
        n = embeds.shape[0]
        if N + n >= 2 ** 31:
            raise _ffi.GdrError("add_documents: doc ids must fit int32")
        embeds = embeds.to(dev).contiguous()
        fc = self._freeze_centroids()
        tgt = fc.assign(embeds, compact=True)
        # doc_embed: append into a geometrically grown buffer (a 64-doc add does not copy the corpus)
        buf = getattr(self, "_doc_buf", None)
        if buf is None or buf.shape[0] < N + n or buf.data_ptr() != self.doc_embed.data_ptr():
            buf = torch.empty((max(N + n, N + N // 2 + 64), d), dtype=torch.float32, device=dev)
            buf[:N].copy_(self.doc_embed)
            self._doc_buf = buf
        buf[N:N + n].copy_(embeds)
        self.doc_embed = buf[:N + n]
        if self.doc_tokens is not None:
            self._append_tokens(tok, msk)
        ids = torch.arange(N, N + n, dtype=torch.int32, device=dev)
        dci = self._device_index()
        C_ = len(self.index.names)
        if dci is not None:
            dci.insert(ids, tgt, target_map=fc.cmap, streams=getattr(self, "_streams", ()))
            offs, mem = dci.offsets, dci.members[:dci.n_members]
        else:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
            offs, mem, _mx = ops.cluster_insert(up(self.index.offsets), up(self.index.members), ids, tgt, fc.cmap)
        csr = torch.cat([offs, mem]).cpu().numpy()                                  # one read-back of the merged CSR
        self.index = self.index.with_csr(csr[:C_ + 1], csr[C_ + 1:])
        if getattr(self, "_live", None) is not None:
            self._live.grow(N + n).set(ids)
        if getattr(self, "_prefiltered", None) is not None:
            self._prefiltered.rebind(self.doc_embed)                 # the new rows' image; the old rows keep theirs
        return np.arange(N, N + n, dtype=np.int64), fc.cmap[tgt.long()].cpu().numpy()

    def _document_rows(self, what, embeds, tokens):
        """The embeds= / tokens= arguments of add_documents and update_documents, validated: (embeds fp32 [n, d] — embedded by
        the doc tower when only tokens were given —, input_ids, attention_mask on the device or None, None)."""
        dev = self.doc_embed.device
        d = self.doc_embed.shape[1]
        tok = msk = None
        if self.doc_tokens is not None and tokens is None:
            raise _ffi.GdrError(f"{what}: the re-encode path is configured (doc_tokens=): pass tokens= as well")
        if tokens is not None:
            tok, msk = (t.to(dev) for t in tokens)
            if tok.dim() != 2 or msk.shape != tok.shape:
                raise _ffi.GdrError(f"{what}: tokens {tuple(tok.shape)} / mask {tuple(msk.shape)} must be [n, Lp]")
        if embeds is None:
            if tokens is None:
                raise _ffi.GdrError(f"{what}: pass embeds= or tokens=")
            if getattr(self.encoder, "bert", None) is None:
                raise _ffi.GdrError(f"{what}(tokens=...) needs the doc tower (doc_tower=)")
            embeds = self.encoder(passage={"input_ids": tok, "attention_mask": msk})
        embeds = torch.as_tensor(embeds)
        if embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[1] != d:
            raise _ffi.GdrError(f"{what}: embeds must be fp32 [n, {d}], got {embeds.dtype} {tuple(embeds.shape)}")
        n = embeds.shape[0]
        if tokens is not None and tok.shape[0] != n:
            raise _ffi.GdrError(f"{what}: {n} embeddings but {tok.shape[0]} token rows")
        return embeds, tok, msk

    def _lifecycle_ids(self, what, ids):
        """The refusals remove_documents / update_documents share with add_documents, then `ids` as int64 numpy in [0, N)."""
        import numpy as np
        if self.sharded is not None:
            raise _ffi.GdrError(f"{what}: a sharded retriever cannot change its documents (sharded removal is not supported)")
        if self.doc_embed is None or self.doc_embed.dtype != torch.float32:
            raise _ffi.GdrError(f"{what} needs the fp32 doc_embed (the bf16 precision mode is not supported)")
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise _ffi.GdrError(f"{what}: ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64)
        N = self.doc_embed.shape[0]
        if ids.size and (ids.min() < 0 or ids.max() >= N):
            raise _ffi.GdrError(f"{what}: doc ids must lie in [0, {N})")
        return ids

    def _freeze_centroids(self):
        """The centroids every add / remove / update uses, computed before the first of them touches the index."""
        if getattr(self, "_centroids", None) is None:
            self._centroids = ops.FrozenCentroids(self.doc_embed, self.index)          # frozen: the index as built
        return self._centroids

    def _edit_csr(self, remove, insert=None, targets=None):
        """Removes the ascending int32 ids `remove` from the member CSR and then, if given, inserts `insert` (ascending) into
        the compact targets `targets` of the frozen centroids; replaces the device index and the host ClusterIndex (one
        read-back), as add_documents does.  Returns the number of ids removed."""
        import numpy as np
        dev = self.doc_embed.device
        fc = self._centroids
        dci = self._device_index()
        streams = getattr(self, "_streams", ())
        if dci is not None:
            gone = dci.remove(remove, streams=streams)
            if insert is not None:
                dci.insert(insert, targets, target_map=fc.cmap, streams=streams)
            offs, mem = dci.offsets, dci.members[:dci.n_members]
        else:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
            offs, mem, _mx, gone = ops.cluster_remove(up(self.index.offsets), up(self.index.members), remove)
            if insert is not None:
                offs, mem, _mx = ops.cluster_insert(offs, mem, insert, targets, fc.cmap)
        C_ = len(self.index.names)
        csr = torch.cat([offs, mem]).cpu().numpy()                                  # one read-back of the edited CSR
        self.index = self.index.with_csr(csr[:C_ + 1], csr[C_ + 1:])
        return gone

    @torch.no_grad()
    def remove_documents(self, ids):
        """Withdraws documents from the index: `ids` (any integer array-like, sorted and de-duplicated here, each in [0, N))
        leave their clusters and are never stage-2 candidates again.  Their rows of doc_embed / doc_tokens stay where they
        are — doc ids are row numbers and never shift.  An id that is in no cluster (removed earlier) is ignored.  Every
        cluster keeps its other members in their order; a cluster that loses all of them stays, empty, keeps its frozen
        centroid and can receive documents again (add_documents / update_documents).  The centroids are frozen from the index
        as built before the first add / remove / update touches it, so the order of those calls never changes them.  Both the
        device index and the host ClusterIndex are replaced (one read-back).  Returns the number of documents removed.
        Must not run while validation_steps() has steps in flight.  Raises GdrError for a sharded retriever, a bf16
        doc_embed and an id outside [0, N); nothing has changed then."""
        import numpy as np
        ids = np.unique(self._lifecycle_ids("remove_documents", ids))
        self._freeze_centroids()
        if ids.size == 0:
            return 0
        gone = self._edit_csr(torch.from_numpy(ids.astype(np.int32)).to(self.doc_embed.device))
        if getattr(self, "_live", None) is not None:
            self._live.clear(ids)
        return gone

    @torch.no_grad()
    def update_documents(self, ids, embeds=None, tokens=None):
        """Re-writes documents in place: row ids[i] of doc_embed becomes embeds[i] (embeds= / tokens= as in add_documents; with
        the re-encode path configured the rows of doc_tokens are overwritten too, and doc_tokens is widened once when a new
        passage is longer than every earlier one), the ids leave the clusters they are in and join the cluster of the
        nearest frozen centroid, exactly as a document added with that embedding would.  An id that is in no cluster (removed
        earlier) is thereby restored.  `ids`: distinct doc ids in [0, N), in any order.  Returns the cluster index of each,
        int32[n], in the order of `ids`.
        Must not run while validation_steps() has steps in flight.  Raises GdrError for a sharded retriever, a bf16
        doc_embed, ids that repeat or lie outside [0, N), and embeds / tokens that do not fit; nothing has changed then."""
        import numpy as np
        ids = self._lifecycle_ids("update_documents", ids)
        dev = self.doc_embed.device
        embeds, tok, msk = self._document_rows("update_documents", embeds, tokens)
        if embeds.shape[0] != ids.size:
            raise _ffi.GdrError(f"update_documents: {ids.size} ids but {embeds.shape[0]} embeddings")
        order = np.argsort(ids, kind="stable")
        if np.any(np.diff(ids[order]) == 0):
            raise _ffi.GdrError("update_documents: an id is given twice")
        fc = self._freeze_centroids()
        if ids.size == 0:
            return np.zeros(0, np.int32)
        sel = torch.from_numpy(order).to(dev)
        rows = torch.from_numpy(ids[order]).to(dev)                                 # ascending int64
        embeds = embeds.to(dev).index_select(0, sel).contiguous()
        tgt = fc.assign(embeds, compact=True)
        self.doc_embed.index_copy_(0, rows, embeds)
        if self.doc_tokens is not None:
            self._overwrite_tokens(rows, tok.index_select(0, sel), msk.index_select(0, sel))
        ids32 = rows.to(torch.int32)
        self._edit_csr(ids32, insert=ids32, targets=tgt)
        if getattr(self, "_live", None) is not None:
            self._live.set(rows)
        if getattr(self, "_prefiltered", None) is not None:
            self._prefiltered.update_rows(rows)                      # (remove_documents needs nothing: a withdrawn row is masked)
        out = np.empty(ids.size, np.int32)
        out[order] = fc.cmap[tgt.long()].cpu().numpy()
        return out

    @torch.no_grad()
    def compact_documents(self, chunk_rows=0):
        """Reclaims the rows of the removed documents: the live rows (live_rows: the members of some cluster) move to the front of
        doc_embed in their order and ARE the corpus from here on — doc ids are renumbered, old id r becomes plan.new_id[r].
        Compacted in place on the device (ops.RowCompaction.rows; chunk_rows bounds the bounce buffer, 0 = the library default):
        doc_embed in its backing buffer, which keeps its capacity while the view shrinks (the next add_documents appends behind
        the live rows without a reallocation); both doc_tokens tables when configured; the pre-filter image when one was built
        (its rows move, its norm bound is kept).  Renumbered: the device index's member list and the host ClusterIndex (one
        read-back of the CSR, as the other lifecycle calls do; names and offsets unchanged).  live_rows becomes all-live over the
        new rows.  The frozen centroids stay: the map is monotone, so every cluster's ascending member order and the member rows'
        values are what they were, and centroids frozen after a compaction have the bits of centroids frozen before it.
        Returns the ops.RowCompaction (new_id / old_id on the device; .ids() renumbers results a caller still holds).  With nothing
        dead it is an identity plan and nothing was touched.
        Must not run while validation_steps() has steps in flight.  Raises GdrError for a sharded retriever, a bf16 doc_embed
        and a token table whose row is not a multiple of 4 bytes; nothing has changed then."""
        import numpy as np
        if self.sharded is not None:
            raise _ffi.GdrError("compact_documents: a sharded retriever cannot change its documents (sharded removal is not supported)")
        if self.doc_embed is None or self.doc_embed.dtype != torch.float32:
            raise _ffi.GdrError("compact_documents needs the fp32 doc_embed (the bf16 precision mode is not supported)")
        dev = self.doc_embed.device
        plan = ops.compact_plan(self.live_rows)
        if plan.identity:
            return plan
        # everything that can refuse comes first: the token tables' row size, and the member lists (a member that is no live row)
        tables = [self.doc_embed] + list(self.doc_tokens if self.doc_tokens is not None else ())
        tables = [t if t.is_contiguous() else t.contiguous() for t in tables]
        for t in tables:
            plan._row_bytes("doc_embed" if t is tables[0] else "a doc_tokens table", t)
        dci = self._device_index()
        C_ = len(self.index.names)
        if dci is not None:
            dci.compact(plan)
            offs, mem = dci.offsets, dci.members[:dci.n_members]
        else:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
            offs, mem = up(self.index.offsets), plan.ids(up(self.index.members))
        csr = torch.cat([offs, mem]).cpu().numpy()                                  # one read-back of the renumbered CSR
        self.index = self.index.with_csr(csr[:C_ + 1], csr[C_ + 1:])
        # the rows: each table in place; a table that had no backing buffer yet becomes its own (capacity n_old for later adds)
        if getattr(self, "_doc_buf", None) is None or self._doc_buf.data_ptr() != tables[0].data_ptr():
            self._doc_buf = tables[0]
        self.doc_embed = plan.rows(tables[0], chunk_rows=chunk_rows)
        if self.doc_tokens is not None:
            bt, bm = getattr(self, "_tok_buf", (None, None))
            if bt is None or bt.data_ptr() != tables[1].data_ptr() or bm.data_ptr() != tables[2].data_ptr() or bt.shape[1] != tables[1].shape[1]:
                self._tok_buf = (tables[1], tables[2])
            self.doc_tokens = (plan.rows(tables[1], chunk_rows=chunk_rows), plan.rows(tables[2], chunk_rows=chunk_rows))
        if getattr(self, "_prefiltered", None) is not None:
            self._prefiltered.compact(plan, self.doc_embed)
        self._live = plan.live_rows()
        return plan

    def _overwrite_tokens(self, rows, tok, msk):
        """doc_tokens[rows] = (tok, msk), PAD 0 / mask 0 behind a shorter passage; a longer one widens the buffers first (one
        copy of the token table, as in _append_tokens)."""
        old_t, old_m = self.doc_tokens
        N, L0 = old_t.shape
        L1 = tok.shape[1]
        if L1 > L0:
            bt, bm = getattr(self, "_tok_buf", (None, None))
            live = bt is not None and bt.data_ptr() == old_t.data_ptr() and bm.data_ptr() == old_m.data_ptr() and bt.shape[1] == L0
            cap = bt.shape[0] if live else N
            bt = torch.zeros((cap, L1), dtype=old_t.dtype, device=old_t.device)
            bm = torch.zeros((cap, L1), dtype=old_m.dtype, device=old_m.device)
            bt[:N, :L0].copy_(old_t)
            bm[:N, :L0].copy_(old_m)
            self._tok_buf = (bt, bm)
            self.doc_tokens = (bt[:N], bm[:N])
        dst_t, dst_m = self.doc_tokens
        W = dst_t.shape[1]
        pad = lambda x: torch.nn.functional.pad(x, (0, W - L1))                     # noqa: E731
        dst_t.index_copy_(0, rows, pad(tok.to(dst_t.dtype)))
        dst_m.index_copy_(0, rows, pad(msk.to(dst_m.dtype)))

    def _append_tokens(self, tok, msk):
        """doc_tokens += (tok, msk) in backing buffers grown like doc_embed's: rows geometrically, and once wider when a passage is
        longer than every earlier one (PAD 0, mask 0) — an add after the first copies only its own rows."""
        old_t, old_m = self.doc_tokens
        N, L0 = old_t.shape
        n, L1 = tok.shape
        bt, bm = getattr(self, "_tok_buf", (None, None))
        if (bt is None or bt.shape[0] < N + n or bt.shape[1] < L1 or bt.data_ptr() != old_t.data_ptr()
                or bm.data_ptr() != old_m.data_ptr() or bt.shape[1] != L0):
            grow = bt is None or bt.shape[0] < N + n or bt.data_ptr() != old_t.data_ptr()
            cap = max(N + n, N + N // 2 + 64) if grow else bt.shape[0]
            L = max(L0, L1)
            bt = torch.zeros((cap, L), dtype=old_t.dtype, device=old_t.device)
            bm = torch.zeros((cap, L), dtype=old_m.dtype, device=old_m.device)
            bt[:N, :L0].copy_(old_t)
            bm[:N, :L0].copy_(old_m)
            self._tok_buf = (bt, bm)
        W = bt.shape[1]
        bt[N:N + n, :L1].copy_(tok)
        bm[N:N + n, :L1].copy_(msk)
        bt[N:N + n, L1:W].zero_()
        bm[N:N + n, L1:W].zero_()
        self.doc_tokens = (bt[:N + n], bm[:N + n])

    def _reencode(self, cand_ids, chunk=1024):
        """Embeds the candidate docs with the doc tower (main_models.py:1445-1455).  cand_ids int32 [total] on device."""
        tok, msk = self.doc_tokens
        out = []
        for lo in range(0, cand_ids.numel(), chunk):
            sel = cand_ids[lo:lo + chunk].long()
            out.append(self.encoder(passage={"input_ids": tok[sel], "attention_mask": msk[sel]}))
        return torch.cat(out, dim=0)

    @torch.no_grad()
    def validation_step_i(self, batch, i=-1, reencode=False):
        """batch: {"source_ids", "source_mask"} (+ optionally what the reference's dataset adds for the metric rows:
        "texts" list[str] (the reference decodes them from source_ids with the T5 tokenizer — out of scope here),
        "gt" list[str] gold cluster ids, "rank" list[int], "oldid" list[str] gold doc ids).
        Returns the reference's step output {"inf_result_batch", "inf_result_batch_prob", "inf_index_batch"}
        (main_models.py:1640-1641; rows are filled when "texts" is given) plus the raw pieces: "clusters" [B][R] decoded
        cluster strings, "doc_ids" [B][A][R] doc ids as strings, "rerank_values" fp32[B,A,R]."""
        return self._step_finish(self._step_launch(batch), reencode=reencode)

    @torch.no_grad()
    def validation_steps(self, batches, depth=2, reencode=False):
        """The same steps for a sequence of batches with up to `depth` of them in flight, each on a HIP stream of its own:
        while the host decodes batch k's docids, looks up its candidates and formats its rows (the part of
        validation_step_i that needs the beam output on the host, main_models.py:1398-1462), the GPU already runs batch
        k+1's encoder and beam decode; per-stream scratch (ops.Workspace) keeps the calls apart.  Yields the step outputs
        in order — identical to calling validation_step_i batch by batch."""
        if depth <= 1:
            for b in batches:
                yield self.validation_step_i(b, reencode=reencode)
            return
        if not hasattr(self, "_streams") or len(self._streams) < depth:
            self._streams = [torch.cuda.Stream(device=self.model.device) for _ in range(depth)]
        cur = torch.cuda.current_stream(self.model.device)
        pending, k = [], 0
        for b in batches:
            st = self._streams[k % depth]
            st.wait_stream(cur)                              # inputs prepared on the caller's stream
            with torch.cuda.stream(st):
                pending.append((st, self._step_launch(b)))
            k += 1
            if len(pending) == depth:
                st0, state = pending.pop(0)
                with torch.cuda.stream(st0):
                    out = self._step_finish(state, reencode=reencode)
                yield out
        for st0, state in pending:
            with torch.cuda.stream(st0):
                out = self._step_finish(state, reencode=reencode)
            yield out

    def _step_launch(self, batch):
        a = self.args
        self._need_beams(a)
        R = a.num_return_sequences
        mask = batch["source_mask"] if batch.get("source_mask") is not None else torch.ones_like(batch["source_ids"])
        enc_h, ids, lens, scores = self.model._generate_launch(batch["source_ids"], mask, R, a.max_output_length,
                                                               a.length_penalty, R)
        for t in (enc_h, ids, lens, scores):                 # produced on this stream, possibly consumed after a switch
            if t.is_cuda:
                t.record_stream(torch.cuda.current_stream(t.device))
        return {"batch": batch, "enc_h": enc_h, "ids": ids, "lens": lens, "scores": scores}

    def _device_index(self):
        """The cluster index on the GPU (ops.DeviceClusterIndex), built on first use; None when the id scheme has no
        separator (--kary 0): the host lookup below then serves, as in round 2."""
        if not hasattr(self, "_dci"):
            a = self.args
            self._dci = None
            if getattr(a, "kary", 30) and self.device_candidates:
                dev = self.model.device if self.model is not None else self.doc_embed.device
                self._dci = ops.DeviceClusterIndex(self.index, dev, getattr(a, "output_vocab_size", a.kary),
                                                   position=getattr(a, "position", 1), kary=a.kary)
        return self._dci

    def _decoder_queries(self, state):
        """The decoder-side stage-2 queries, fp32[B*R, d]: the decoder runs over the step's own hypotheses (ops.T5DecoderHandle.score
        on state["ids"], already on the device) and every hypothesis brings its last hidden state at the EOS position
        (use_query_embed_decoder_special, main_models.py:1568-1571) or the mean over its tokens (use_query_embed_decoder_avg,
        :1469-1476,1507).  A hypothesis that never emitted EOS has no `special` vector — the reference's boolean gather then
        returns fewer rows than hypotheses and every later row meets another hypothesis' candidates; here it raises.  That check reads
        one number back before the rerank is enqueued (the encoder-CLS path and `avg` enqueue everything first), so `special`
        overlaps less across the batches of validation_steps(depth > 1)."""
        a = self.args
        mask = state["batch"].get("source_mask")
        mask = torch.ones_like(state["batch"]["source_ids"]) if mask is None else mask
        _scores, _trace, at_eos, mean = self.model.dec.score(state["enc_h"], mask.to(state["enc_h"].device), state["ids"],
                                                            a.num_return_sequences, a.length_penalty, hidden=True)
        if self.query_form == "avg":
            return mean
        open_rows = int((~(state["ids"][:, 1:] == 1).any(dim=1)).sum().item())
        if open_rows:
            raise _ffi.GdrError(f"use_query_embed_decoder_special: {open_rows} of {state['ids'].shape[0]} decoded hypotheses never "
                                "emitted EOS and have no EOS hidden state to query with (constrain the decode with the docid trie, "
                                "or use use_query_embed_decoder_avg)")
        return at_eos

    def _step_finish(self, state, reencode=False):
        a = self.args
        R = a.num_return_sequences
        batch = state["batch"]
        row_queries = self.query_form != "encoder"
        if row_queries:
            query_embeds = self._decoder_queries(state)                         # [B*R, d] (main_models.py:1467-1571)
            B = query_embeds.shape[0] // R
        else:
            query_embeds = self.encoder(query_enc=state["enc_h"]).contiguous()  # CLS rows (main_models.py:1466)
            B = query_embeds.shape[0]
        alphas, func = list(a.score_rate), getattr(a, "loss_func", "tanh")
        dci = self._device_index()
        stride = 0
        if dci is not None:
            # decode_token -> id_mapping -> candidate lists -> rerank, all enqueued before anything is read back
            # (main_models.py:1398,1441-1443,1574-1637): the host only formats strings afterwards
            _cl, offs, dev_ids, stride = dci.candidates(state["ids"], B, R)
            # the sharded stage 2 takes its bound from the GATHERED offsets (dist.ShardedIndex): a rank-local decision here could
            # raise on one rank while its peers already sit in the fixed-size all-gather
            max_cand = 0 if self.sharded is not None else ops.block_max_cand(offs, R, stride, cap=ops.RERANK_LONG_MAX_CAND)
            beam_scores = state["scores"].to(torch.float32).view(B, R)          # fp64 -> fp32 as torch.tensor(list) rounds
        outs = scores = None
        if dci is None:
            outs, scores = ops.finish_generate_output(state["ids"], state["lens"], state["scores"], a.max_output_length)
            dec = codec.dec_2d(codec.decode_token(a, outs.cpu().numpy()), R)
            offs, ids, max_cand = self.index.candidates(dec)
            offs = offs.to(query_embeds.device)
            beam_scores = torch.tensor(scores, dtype=torch.float32, device=query_embeds.device).view(B, R)
            dev_ids = ids.to(query_embeds.device)
        if self.sharded is not None:
            if dci is None or reencode:
                raise _ffi.GdrError("the sharded two-stage path needs the device cluster index (--kary > 0) and has no "
                                    "re-encode form (the doc tower's tokens are not sharded)")
            vals, idx = self.sharded.rerank_own(query_embeds, offs, dev_ids, beam_scores, alphas, R, func=func)
        elif reencode:
            if self.doc_tokens is None or getattr(self.encoder, "bert", None) is None:
                raise _ffi.GdrError("re-encode needs doc_tower= and doc_tokens=")
            if stride:                                   # block layout: the live ids of every query, query-major
                cnt = offs[:, R].long()
                live_mask = torch.arange(stride, device=cnt.device)[None, :] < cnt[:, None]
                live = dev_ids[live_mask]
                start = torch.cumsum(cnt, 0) - cnt
                local = (start[:, None] + torch.arange(stride, device=cnt.device)[None, :]).to(torch.int32)
            else:
                live = dev_ids[:max(int(offs[-1].item()), 1)]
                local = torch.arange(live.numel(), dtype=torch.int32, device=dev_ids.device)
            if live.numel() == 0:
                live = dev_ids.reshape(-1)[:1]
            cand_embeds = self._reencode(live)                                      # [total, d], candidate order
            vals, pos = ops.rerank_topk(query_embeds, cand_embeds, offs, local, beam_scores, alphas, R, func=func,
                                        max_cand=max_cand, cand_stride=stride, row_queries=row_queries)
            idx = torch.where(pos >= 0, live[pos.clamp(min=0).long()], pos)         # candidate position -> doc id
        else:
            vals, idx = ops.rerank_topk(query_embeds, self.doc_embed, offs, dev_ids, beam_scores, alphas, R, func=func,
                                        max_cand=max_cand, cand_stride=stride, row_queries=row_queries)
        if outs is None:                                                            # first read-back of the step
            outs, scores = ops.finish_generate_output(state["ids"], state["lens"], state["scores"], a.max_output_length)
        outs_h = outs.cpu().numpy()
        idx_np = idx.cpu().numpy()                                                  # [B, A, R] doc ids (-1 = padding)
        _ffi.check_device_fault("validation_step_i")             # everything of this step has been read back
        A = len(a.score_rate)
        if dci is not None:
            dec = LazyRows(B, lambda: codec.dec_2d(codec.decode_token(a, outs_h), R))
        doc_ids = LazyRows(B, lambda: [[list(map(str, row)) for row in q] for q in idx_np.tolist()])
        inf_result, inf_index = [], []
        texts = batch.get("texts")
        if texts is not None:
            gts = batch.get("gt", [""] * B)
            ranks = batch.get("rank", [1] * B)
            old = batch.get("oldid", [""] * B)
            idx_h = idx_np.tolist()
            for b in range(B):                                   # main_models.py:1421-1432 and :1626-1637
                inf_result.append([texts[b], ",".join(dec[b]), gts[b], int(ranks[b])])
                inf_index.append([[[texts[b], ",".join(map(str, idx_h[b][ai])), old[b]]] for ai in range(A)])
        return {"inf_result_batch": inf_result, "inf_result_batch_prob": scores, "inf_index_batch": inf_index,
                "clusters": dec, "doc_ids": doc_ids, "rerank_values": vals, "doc_id_tensor": idx}
