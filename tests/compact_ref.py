"""Numpy restatement of the corpus compaction (include/gdr_hip_compact.h): np.nonzero, fancy indexing and bit
repacking — what tests/test_gpu_compact.py holds the device calls to, integer for integer and byte for byte."""
import numpy as np


def pack(bits):
    """bool [..., n] -> int32 [..., ceil(n / 32)] in LiveRows' / QueryRows' format (bit r % 32 of word r // 32); pad bits are 0."""
    bits = np.asarray(bits, bool)
    n = bits.shape[-1]
    pad = np.zeros(bits.shape[:-1] + (-n % 32,), bool)
    b = np.concatenate([bits, pad], -1).reshape(bits.shape[:-1] + (-1, 32))
    return (b.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


def unpack(words, n):
    """int32 [..., W] -> bool [..., n]."""
    w = np.asarray(words).view(np.uint32)
    bits = (w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[:-1] + (-1,))[..., :n].astype(bool)


def plan(live):
    """live bool [N] -> (new_id int32[N]: the new row or -1, old_id int32[n_live]: the live rows, ascending)."""
    live = np.asarray(live, bool)
    old_id = np.nonzero(live)[0].astype(np.int32)
    new_id = np.full(live.size, -1, np.int32)
    new_id[old_id] = np.arange(old_id.size, dtype=np.int32)
    return new_id, old_id


def rows(table, old_id):
    """table [N, ...] -> its live rows, in order."""
    return np.asarray(table)[old_id]


def rows_in_place(table, old_id):
    """What the in-place form leaves in the whole table: the live rows in front, rows >= n_live as they were."""
    out = np.array(table, copy=True)
    out[:len(old_id)] = np.asarray(table)[old_id]
    return out


def remap(new_id, ids):
    """(out, status): out[i] = new_id[ids[i]]; a negative id stays; an id >= N or a dead row's becomes -1 and sets status."""
    ids = np.asarray(ids, np.int64)
    N = len(new_id)
    ok = (ids >= 0) & (ids < N)
    out = np.where(ids < 0, ids, -1)
    out[ok] = new_id[ids[ok]]
    return out.astype(np.int32), int(((ids >= 0) & (out < 0)).any())


def rowmask(allowed, old_id):
    """allowed bool [B, N] -> the packed bitmaps int32 [B, ceil(n_live / 32)] over the compacted rows."""
    return pack(np.asarray(allowed, bool)[:, old_id])


def index_members(members, new_id):
    """The member list of a cluster index after the compaction: every member mapped, order kept."""
    out = new_id[np.asarray(members, np.int64)]
    assert (out >= 0).all(), "a cluster member is a dead row"
    return out.astype(np.int32)


def compose(first_new_id, second_new_id):
    """new_id of two compactions in a row."""
    out = np.full(first_new_id.size, -1, np.int32)
    ok = first_new_id >= 0
    out[ok] = second_new_id[first_new_id[ok]]
    return out
