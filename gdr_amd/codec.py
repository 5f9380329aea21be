"""Host logic around the kernels: docid codec, cluster index (CSR), retrieval metrics, res1 TSV.

Mirrors the reference's names and argument meaning so call sites read the same:
  encode_single_newid / decode_token   GDR_model/main_models.py:297-346
  dec_2d                               GDR_model/main_utils.py:70-76
  recall / MRR100                      GDR_model/main_metrics.py:194-267
  cal_recall / cal_accuracy / cal_MRR / cal_MAP, validation_epoch_end
                                       GDR_model/main_models.py:1643-1908 (multi-gt macro/micro metrics per alpha)
  id_mapping (cluster -> doc ids)      GDR_model/main_models.py:874-889  -> flat CSR here
Both call styles are accepted: the reference's `f(args, x)` with an argparse namespace, or `f(x, kary=..)`.
"""
import numpy as np
import torch


def _split_args(a, b, **kw):
    """(args, x) or (x, **kw) -> (x, kary, output_vocab_size, position)."""
    if b is not None and hasattr(a, "kary"):
        return b, a.kary, getattr(a, "output_vocab_size", a.kary or 10), getattr(a, "position", 1)
    return a, kw.get("kary", 30), kw.get("output_vocab_size", kw.get("kary", 30) or 10), kw.get("position", 1)


def encode_single_newid(a, b=None, **kw):
    """'3-17-5' -> [5, 49, 67, 1]: token = i*kary + c_i + 2, EOS(1) appended (main_models.py:297-319)."""
    seq, kary, _v, position = _split_args(a, b, **kw)
    out = []
    if kary:
        for i, c in enumerate(seq.split("-")):
            out.append(i * kary + int(c) + 2 if position else int(c) + 2)
    else:
        for i, c in enumerate(seq):
            out.append(i * 10 + int(c) + 2 if position else int(c) + 2)   # hard-coded vocab 10 as in the reference
    return out + [1]


_DIGIT_TABLES = {}


def _digit_table(width, V, position, hi):
    """T[i][t] = str(t - (i*V + 2)) (or str(t - 2)): the printed digit of token t at body position i, for t < hi."""
    key = (width, V, position, hi)
    T = _DIGIT_TABLES.get(key)
    if T is None:
        T = _DIGIT_TABLES[key] = [[str(t - ((i * V + 2) if position else 2)) for t in range(hi)] for i in range(width)]
    return T


def decode_token(a, b=None, **kw):
    """2-D int array of generated ids -> docid strings (main_models.py:322-346): drop START, cut at the first
    EOS, subtract arange*V+2.  A row without EOS is decoded whole, START included, as the reference does."""
    seqs, kary, V, position = _split_args(a, b, **kw)
    if torch.is_tensor(seqs):
        seqs = seqs.cpu().numpy()
    arr = np.asarray(seqs)
    sep = "-" if kary else ""
    rows = arr.tolist()                          # plain Python ints: str() of numpy scalars dominated this loop
    result = []
    if arr.ndim == 2 and arr.size and int(arr.min()) >= 0 and int(arr.max()) < 4096:
        # the strings of every (position, token) pair come from a table built once: 3x faster than str() per digit on the
        # 640 rows of a C3 batch (the host part of validation_step_i)
        T = _digit_table(arr.shape[1], V, position, int(arr.max()) + 1 if int(arr.max()) >= 512 else 512)
        getitem = list.__getitem__
        for lst in rows:
            body = lst[1:lst.index(1)] if 1 in lst else lst
            result.append(sep.join(map(getitem, T, body)))
        return result
    for lst in rows:
        body = lst[1:lst.index(1)] if 1 in lst else lst
        if position:
            result.append(sep.join([str(t - (i * V + 2)) for i, t in enumerate(body)]))
        else:
            result.append(sep.join([str(t - 2) for t in body]))
    return result


def dec_2d(dec, size):
    return [dec[i:i + size] for i in range(0, len(dec), size)]


class ClusterIndex:
    """cluster-id string -> member doc ids, as flat CSR (offsets int32[n+1], members int32[N]).
    Replaces the reference's pickled dict `id_mapping` (main_models.py:874-889)."""

    def __init__(self, names, offsets, members):
        self.names = list(names)
        self.offsets = np.asarray(offsets, dtype=np.int32)
        self.members = np.asarray(members, dtype=np.int32)
        self.lookup = {n: i for i, n in enumerate(self.names)}

    @staticmethod
    def from_id_mapping(id_mapping):
        names = list(id_mapping)
        lens = [len(id_mapping[n]) for n in names]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        members = np.concatenate([np.asarray(id_mapping[n], dtype=np.int32) for n in names]) if names else np.zeros(0, np.int32)
        return ClusterIndex(names, offsets, members)

    def with_csr(self, offsets, members):
        """The same clusters (names unchanged) over another member CSR, e.g. the merged one of an insertion."""
        if len(offsets) != len(self.names) + 1:
            raise ValueError(f"{len(offsets) - 1} segments for {len(self.names)} clusters")
        return ClusterIndex(self.names, offsets, members)

    def sorted_members(self):
        """members with every cluster's segment in ascending doc-id order (the order in which the reference's TreeBuilder
        attaches documents, main_models.py:137-151: the rows of title_content.tsv)."""
        seg = np.repeat(np.arange(len(self.names), dtype=np.int64), np.diff(self.offsets))
        return np.ascontiguousarray(self.members[np.lexsort((self.members, seg))], dtype=np.int32)

    def unassigned(self, lo, hi):
        """Doc ids in [lo, hi) that are members of no cluster, ascending."""
        return np.setdiff1d(np.arange(lo, hi, dtype=np.int64), self.members.astype(np.int64)).astype(np.int32)

    def save_npz(self, path):
        """Writes the clusters.npz layout of tools/convert_artifacts.py (cluster_names, cluster_offsets, cluster_members) to
        exactly `path`."""
        with open(path, "wb") as f:
            np.savez(f, cluster_names=np.array(self.names), cluster_offsets=self.offsets, cluster_members=self.members)

    def __getitem__(self, name):
        c = self.lookup.get(name)
        if c is None:
            return []                       # unknown / undecodable cluster: empty segment
        return self.members[self.offsets[c]:self.offsets[c + 1]].tolist()

    def token_bodies(self, V, position=1, kary=30):
        """For every cluster name the token body whose decode_token() image is that name — the inverse of
        main_models.py:322-346 with separator '-': token_i = x_i + (i*V + 2 if position else 2) — or None when no token
        sequence prints as the name (not a '-'-joined list of canonical integers: such a name can never be decoded, the
        reference's dict would simply never be asked for it).  '' is the empty body (a row START, EOS)."""
        if not kary:
            raise ValueError("token_bodies needs a '-'-separated id scheme (--kary > 0)")
        out = []
        for name in self.names:
            if name == "":
                out.append([])
                continue
            xs, i, n, ok = [], 0, len(name), True
            while i < n:
                j = i + 1 if name[i] == "-" else i
                e = j
                while e < n and name[e].isdigit():
                    e += 1
                if e == j or (e < n and name[e] != "-") or e == n - 1:   # no digits / junk / trailing separator
                    ok = False
                    break
                xs.append(int(name[i:e]))
                i = e + 1
            if not ok or "-".join(str(x) for x in xs) != name:
                out.append(None)
                continue
            out.append([x + (k * V + 2 if position else 2) for k, x in enumerate(xs)])
        return out

    def candidates(self, dec):
        """dec: list[B] of list[R] cluster strings -> (cand_offsets int32[B*R+1], cand_ids int32[total], max per query)
        in the order validation_step_i builds them (main_models.py:1441-1443)."""
        offs, ids, max_cand = [0], [], 0
        for row in dec:
            start = offs[-1]
            for name in row:
                c = self.lookup.get(name)
                if c is not None:
                    ids.append(self.members[self.offsets[c]:self.offsets[c + 1]])
                    offs.append(offs[-1] + int(self.offsets[c + 1] - self.offsets[c]))
                else:
                    offs.append(offs[-1])
            max_cand = max(max_cand, offs[-1] - start)
        ids = np.concatenate(ids) if ids else np.zeros(0, np.int32)
        if ids.size == 0:
            ids = np.zeros(1, np.int32)
        return torch.from_numpy(np.asarray(offs, dtype=np.int32)), torch.from_numpy(ids.astype(np.int32)), max_cand


class Trie:
    """Prefix tree over docid token sequences = the reference's TreeBuilder / Node (main_models.py:112-151), flattened:
    child int32[n_nodes, V] (next node for digit c at the node's depth, -1 if absent), eos_ok int32[n_nodes]."""

    def __init__(self, child, eos_ok, V):
        self.child, self.eos_ok, self.V = child, eos_ok, V

    @staticmethod
    def from_sequences(seqs, V):
        """seqs: token lists without START, with trailing EOS(1); a PAD(0) ends a sequence (TreeBuilder.add :135-151).
        Tokens carry their positional offset: token = depth*V + c + 2 (encode_single_newid with --position 1)."""
        child, eos = [[-1] * V], [0]
        for seq in seqs:
            cur = 0
            for depth, tok in enumerate(int(t) for t in seq):
                if tok == 0:
                    break
                if tok == 1:
                    eos[cur] = 1
                    break                     # nothing follows EOS in an encoded id
                c = tok - (depth * V + 2)
                if not 0 <= c < V:
                    raise ValueError(f"token {tok} is not a digit of depth {depth} for V={V}")
                if child[cur][c] < 0:
                    child[cur][c] = len(child)
                    child.append([-1] * V)
                    eos.append(0)
                cur = child[cur][c]
        return Trie(np.asarray(child, dtype=np.int32), np.asarray(eos, dtype=np.int32), V)

    @staticmethod
    def from_docids(docids, V):
        return Trie.from_sequences([encode_single_newid(s, kary=V) for s in docids], V)

    def breadth_first(self):
        """The same trie with nodes renumbered in breadth-first order (root = 0, every depth a contiguous id range — what
        the device prefix table needs, gdr_hip.h GdrPrefixTable) plus its level structure:
        (trie, level_off int32[n_levels+1], parent int32[n], tok int64[n]) where tok[node] is the token that leads to
        the node (depth_of_parent*V + c + 2; root: START = 0)."""
        V, n = self.V, self.child.shape[0]
        order, parent, tok, level_off = [0], [-1], [0], [0, 1]
        new_id = np.full(n, -1, dtype=np.int64)
        new_id[0] = 0
        lo, depth = 0, 0
        while lo < len(order):
            hi = len(order)
            for pos in range(lo, hi):
                kids = self.child[order[pos]]
                for c in np.nonzero(kids >= 0)[0]:
                    new_id[kids[c]] = len(order)
                    order.append(int(kids[c]))
                    parent.append(pos)
                    tok.append(depth * V + int(c) + 2)
            if len(order) > hi:
                level_off.append(len(order))
            lo, depth = hi, depth + 1
        order = np.asarray(order)
        child = self.child[order]
        child = np.where(child >= 0, new_id[np.maximum(child, 0)], -1).astype(np.int32)
        t = Trie(np.ascontiguousarray(child), np.ascontiguousarray(self.eos_ok[order]).astype(np.int32), V)
        return t, np.asarray(level_off, np.int32), np.asarray(parent, np.int32), np.asarray(tok, np.int64)


# ------------------------------------------------------------------------------------------ metrics / res1 TSV
def write_res1(path, rows):
    """rows: (query, pred_csv, gt_csv, rank) — the reference's res1 TSV (main.py:244-247)."""
    with open(path, "w") as f:
        for q, pred, gt, rank in rows:
            f.write(f"{q}\t{pred}\t{gt}\t{rank}\n")


def _read_res1(path):
    with open(path, "r") as f:
        for line in f.readlines():
            yield line[:-1].split("\t")


def recall(args=None, rows=None, recall_num=None, verbose=True):
    """hit@k averaged over queries (main_metrics.py:194-250, non-trivia and trivia branches are identical).
    Accepts the reference call `recall(args)` (reads args.res1_save_path / args.recall_num) or rows directly.
    Returns the last recall value like the reference; `recall.last` holds {k: value}."""
    if rows is None:
        rows = list(_read_res1(args.res1_save_path))
        recall_num = args.recall_num
    q_gt, q_pred, prev_q = {}, {}, ""
    for query, pred, gt, _rank in rows:
        if query != prev_q:
            q_pred[query] = pred.split(",")
            prev_q = query
        if query in q_gt:
            if len(q_gt[query]) <= 100:
                q_gt[query].add(gt)
        else:
            q_gt[query] = set(gt.split(","))
    out, recall_avg = {}, 0.0
    for i in recall_num:
        total = 0
        for q in q_pred:
            top = q_pred[q][:int(i)]
            total += 1 if any(p in top for p in q_gt[q]) else 0
        recall_avg = total / len(q_pred)
        out[int(i)] = recall_avg
        if verbose:
            print(f"recall@{i}: {recall_avg}")
    recall.last = out
    return recall_avg


def MRR100(args=None, rows=None, verbose=True):
    """main_metrics.py:253-267."""
    if rows is None:
        rows = list(_read_res1(args.res1_save_path))
    tot, n = 0.0, 0
    for _q, pred, gt, _rank in rows:
        pl = pred.split(",")
        if gt in pl:
            tot += 1 / (pl.index(gt) + 1)
        n += 1
    mrr = tot / n
    if verbose:
        print("MRR100: {}".format(mrr))
    return mrr


# ------------------------------------------------------------------------------------------ validation_epoch_end metrics
def cal_recall(q_pred, q_gt, k):
    """(macro, micro) recall@k over multi-gt queries (main_models.py:1730-1743): macro = mean over queries of
    hits/len(gt); micro = total hits / total gt."""
    total_hit = total_positive = 0
    total_recall = 0
    for q in q_pred:
        top = q_pred[q][:k]
        is_hit = sum(1 for p in q_gt[q] if p in top)
        total_positive += len(q_gt[q])
        total_recall += is_hit / len(q_gt[q])
        total_hit += is_hit
    return total_recall / len(q_pred), total_hit / total_positive


def cal_accuracy(q_pred, q_gt, k):
    """Share of queries with any gt among their first k predictions (main_models.py:1745-1756)."""
    return sum(1 for q in q_pred if any(p in q_gt[q] for p in q_pred[q][:k])) / len(q_pred)


def cal_MRR(q_pred, q_gt, k):
    """Mean reciprocal rank of the first gt hit within k (main_models.py:1758-1772)."""
    total = 0
    for q in q_pred:
        for rank, p in enumerate(q_pred[q][:k], start=1):
            if p in q_gt[q]:
                total += 1 / rank
                break
    return total / len(q_pred)


def cal_MAP(q_pred, q_gt, k):
    """The reference's MAP@k (main_models.py:1774-1789): sum over hits of (hit number / rank), divided by k (not by the
    number of relevant docs) — kept as written."""
    total = 0
    for q in q_pred:
        pred_true, local = 1, 0
        for rank, p in enumerate(q_pred[q][:k], start=1):
            if p in q_gt[q]:
                local += pred_true / rank
                pred_true += 1
        total += local / k
    return total / len(q_pred)


def _group_rows(rows, gt_as_list, strict=True):
    """The q_pred / q_gt dictionaries validation_epoch_end builds from consecutive rows (main_models.py:1697-1728).
    Cluster rows keep the first row's gt LIST and `.add` on a repeat (an AttributeError in the reference, reached only
    when a query text repeats); doc rows append.  strict=False (what the entry point passes): a repeated query text
    appends its gt instead of raising — a deliberate deviation so that an eval run over real data, where texts can repeat,
    still ends with metrics after all the GPU work is done."""
    q_gt, q_pred, prev = {}, {}, ""
    for row in rows:
        query, pred, gt = row[0], row[1], row[2]
        if query != prev:
            q_pred[query] = pred.split(",")
            prev = query
        if query in q_gt:
            if len(q_gt[query]) <= 100:
                if gt_as_list or not strict:
                    q_gt[query].append(gt)
                else:
                    q_gt[query].add(gt)          # the reference calls set.add on a list here (main_models.py:1708)
        else:
            q_gt[query] = list(set(gt.split(",")))
    return q_pred, q_gt


def validation_epoch_end(outputs, args, verbose=False, strict=True):
    """The metric block of T5FineTuner.validation_epoch_end (main_models.py:1643-1908) for multiple_decoder=0.
    outputs: list of validation_step_i results {"inf_result_batch": [[query, pred_csv, gt, rank], ...],
    "inf_result_batch_prob": [...], "inf_index_batch": [batch][alpha] -> [[query, pred_csv, gt]]}.
    Returns the dict of everything the reference passes to self.log (same names, e.g. "cluster_recall10",
    "recall5_0.5", "MRR100_3", "MAP100_1.5"; without is_train_encoder: "recall1" ... "MAP100")."""
    logged = {}
    n_alpha = len(outputs[0]["inf_index_batch"][0]) if args.is_train_encoder else 1
    for index in range(n_alpha):
        appendix = args.score_rate[index]
        rows = [item for sub in outputs for item in sub["inf_result_batch"]]
        rows = sorted((r for r in rows), key=lambda r: (r[0], r[3]))         # sort_values(by=['query','rank'])
        q_pred, q_gt = _group_rows([r for r in rows if r[3] == 1], gt_as_list=False, strict=strict)
        ks = (1, 5, 10, 20, 50, 100)
        if args.is_train_encoder:
            index_rows = [item for sub in outputs for b in range(args.eval_batch_size)
                          for item in sub["inf_index_batch"][b][index]]
            q_pred_i, q_gt_i = _group_rows(index_rows, gt_as_list=True)
            for k in ks:
                logged[f"cluster_recall{k}"] = cal_recall(q_pred, q_gt, k)[0]
            for k in (1, 20, 100):
                logged[f"cluster_accuracy{k}"] = cal_accuracy(q_pred, q_gt, k)
            logged["cluster_MRR100"], logged["cluster_MRR10"] = cal_MRR(q_pred, q_gt, 100), cal_MRR(q_pred, q_gt, 10)
            logged["cluster_MAP100"] = cal_MAP(q_pred, q_gt, 100)
            for k in ks:
                logged[f"recall{k}_{appendix}"] = cal_recall(q_pred_i, q_gt_i, k)[0]
            if appendix == 0:
                logged["recall1"] = logged[f"recall1_{appendix}"]
            for k in (1, 20, 100):
                logged[f"accuracy{k}_{appendix}"] = cal_accuracy(q_pred_i, q_gt_i, k)
            logged[f"MRR100_{appendix}"], logged[f"MRR10_{appendix}"] = cal_MRR(q_pred_i, q_gt_i, 100), cal_MRR(q_pred_i, q_gt_i, 10)
            logged[f"MAP100_{appendix}"] = cal_MAP(q_pred_i, q_gt_i, 100)
            if verbose:
                for k in ks:
                    print(f"recall@{k}_{appendix}:{logged[f'recall{k}_{appendix}']}")
                print(f"MRR100_{appendix}:{logged[f'MRR100_{appendix}']}")
        else:
            for k in ks:
                logged[f"recall{k}"] = cal_recall(q_pred, q_gt, k)[0]
            for k in (1, 20, 100):
                logged[f"accuracy{k}"] = cal_accuracy(q_pred, q_gt, k)
            logged["MRR100"], logged["MRR10"] = cal_MRR(q_pred, q_gt, 100), cal_MRR(q_pred, q_gt, 10)
            logged["MAP100"] = cal_MAP(q_pred, q_gt, 100)
            if verbose:
                for k in ks:
                    print(f"recall@{k}:{logged[f'recall{k}']}")
                print(f"MRR100:{logged['MRR100']}")
    return logged
