"""Host restatement (numpy) of document removal and update in the member CSR: what
tests/test_lifecycle_host.py checks against hand-written cases and tests/test_gpu_lifecycle.py checks the device code against."""
import numpy as np

import expand_ref


def remove(offsets, members, ids):
    """(offsets int32[C+1], members int32[n_left], n_removed): every cluster keeps, in their order, its members that are not
    in `ids`; a cluster that loses all of them becomes an empty segment; an id that is in no cluster changes nothing."""
    members = np.asarray(members)
    keep = ~np.isin(members, np.asarray(ids).reshape(-1))
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(np.asarray(offsets, np.int64)))
    offs = np.concatenate([[0], np.cumsum(np.bincount(seg[keep], minlength=len(offsets) - 1))])
    return offs.astype(np.int32), members[keep].astype(np.int32), int(members.size - keep.sum())


def update(offsets, members, ids, targets):
    """(offsets, members): the ids leave the clusters they are in (remove), then join their targets by the insertion rule of
    tests/expand_ref.py: behind the cluster's members, in ascending id order."""
    offs, mem, _ = remove(offsets, members, ids)
    return expand_ref.merge(offs, mem, ids, targets)
