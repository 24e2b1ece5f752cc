"""Host dictionary for dense-index engines (``OPT_DENSE_IDS``).

A dense engine's ``key_hash`` column carries small series indices, not the
64-bit series hashes; ``DenseIds`` is the dictionary a host keeps to hand them
out: hash -> index in order of first appearance, starting at 1 (index 0 stays
"no series").  Pure numpy and dict code.
"""
from __future__ import annotations

import numpy as np

#: the id of a span whose series has no index left: past every table's
#: capacity, so the engine counts the span in ``dropped_table_full``
NO_INDEX = 2**64 - 1


class DenseIds:
    """``capacity`` = the engine's ``table_capacity``: indices 1 .. capacity - 1."""

    def __init__(self, capacity: int):
        if capacity < 2:
            raise ValueError("capacity must be at least 2 (index 0 is 'no series')")
        self.capacity = int(capacity)
        self._index = {}      # hash -> index
        self._hash = {}       # index -> hash
        self._next = 1        # the next index never handed out
        self._free = []       # released and flushed: assignable, lowest first
        self._pending = []    # released, not assignable before flushed()

    def __len__(self):
        return len(self._index)

    def index_of(self, key_hash: int) -> int:
        """The index of a hash (0: none)."""
        return self._index.get(int(key_hash), 0)

    def hash_of(self, index: int) -> int:
        """The hash an index stands for (0: none)."""
        return self._hash.get(int(index), 0)

    def _take(self):
        if self._free:
            return self._free.pop(0)
        if self._next < self.capacity:
            self._next += 1
            return self._next - 1
        return None

    def encode(self, key_hash):
        """ids of a batch's hashes, and the (index, hash) pairs assigned by
        this call -- to be bound (``Engine.bind_ids``) before the batch is
        ingested.  Hash 0 -> id 0; a hash with no free index -> ``NO_INDEX``."""
        kh = np.ascontiguousarray(key_hash, dtype=np.uint64)
        uniq, first, inv = np.unique(kh, return_index=True, return_inverse=True)
        uid = np.zeros(len(uniq), dtype=np.uint64)
        new_i, new_h = [], []
        for u in np.argsort(first, kind="stable"):  # new series in order of appearance
            h = int(uniq[u])
            if h == 0:
                continue
            i = self._index.get(h)
            if i is None:
                i = self._take()
                if i is None:
                    uid[u] = NO_INDEX
                    continue
                self._index[h] = i
                self._hash[i] = h
                new_i.append(i)
                new_h.append(h)
            uid[u] = i
        return uid[inv.reshape(-1)], np.array(new_i, dtype=np.uint64), np.array(new_h, dtype=np.uint64)

    def release(self, key_hashes):
        """Frees the indices of these hashes; they become assignable only after
        ``flushed()`` (an index is rebound only with no unflushed spans on it)."""
        for h in np.asarray(key_hashes, dtype=np.uint64).reshape(-1):
            i = self._index.pop(int(h), None)
            if i is not None:
                del self._hash[i]
                self._pending.append(i)

    def flushed(self):
        """The engine was flushed: released indices may be assigned again."""
        if self._pending:
            self._free = sorted(self._free + self._pending)
            self._pending = []
