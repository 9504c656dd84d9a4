"""A cache of decoded examples that stay where they are (train_segnet.py --device_cache_gb): the loaders of
segnet_loader.py decode a frame or a label once and read it from here every later time it comes round.

Storage is a few large allocations (chunks) that are held until close(); an entry is a byte range of one chunk, found
by a key, (zip path, member name) for a frame or a label array of the training loader, so that every loader of a
process shares one cache and one budget.  There is no eviction: entries are admitted in the order they are first seen
until the budget (the bytes of all chunks together) is used, and whatever is not admitted is decoded as before.  An
entry never moves and is never freed before close(): the input kernels read it through its address.

An entry is reserved first (its range is taken, nobody may read it), filled by whoever reserved it, and then
committed; only a committed entry is a hit.  A reservation that is given back (its batch took the host path) leaves
its range to the next reservation of the same size.

DeviceFrameCache keeps the chunks in device memory (torch uint8 tensors), HostFrameCache in numpy arrays: the same
bookkeeping without a GPU, for segnet_loader.HostStage and the CPU tests.  torch is imported by the device variant
only.
"""
import numpy as np

ALIGN = 16                    # entries start on multiples of it; the padding counts against the budget
CHUNK_BYTES = 1 << 30


class Entry(object):
    """chunk, offset, nbytes: where the bytes lie.  committed: they may be read.  owner: who reserved it.  ready: the
    event after which a device entry is filled (None: host).  meta: what the owner keeps with it."""
    __slots__ = ('key', 'chunk', 'offset', 'nbytes', 'committed', 'owner', 'ready', 'meta')

    def __init__(self, key, chunk, offset, nbytes, owner):
        self.key, self.chunk, self.offset, self.nbytes, self.owner = key, chunk, offset, nbytes, owner
        self.committed, self.ready, self.meta = False, None, None


class FrameCache(object):
    """The bookkeeping; a subclass allocates a chunk (_alloc) and says where it lies (address)."""

    def __init__(self, budget_bytes, chunk_bytes=CHUNK_BYTES):
        self.budget = max(int(budget_bytes), 0)
        self.chunk_bytes = max(int(chunk_bytes), ALIGN)
        self.chunks, self.sizes, self.used = [], [], []          # per chunk: storage, size, bytes handed out
        self.table = {}                                          # key -> Entry, reserved or committed
        self.spare = {}                                          # nbytes -> [(chunk, offset)] of returned reservations
        self.full = False                                        # a reservation has been refused: nothing more is admitted
        self.stages = []
        self.hits = self.misses = self.entries = self.bytes = 0
        self.closed = False

    # ---- storage
    def _alloc(self, nbytes):
        raise NotImplementedError

    def _place(self, nbytes):
        """-> (chunk, offset) for nbytes more, or None when the budget does not hold them"""
        if self.spare.get(nbytes):
            return self.spare[nbytes].pop()
        if self.full:
            return None
        padded = -(-nbytes // ALIGN) * ALIGN
        if self.chunks and self.used[-1] + padded <= self.sizes[-1]:
            c = len(self.chunks) - 1
        else:
            left = self.budget - sum(self.sizes)
            size = min(max(self.chunk_bytes, padded), left)
            if size < padded:
                return None
            self.chunks.append(self._alloc(size))
            self.sizes.append(size)
            self.used.append(0)
            c = len(self.chunks) - 1
        off = self.used[c]
        self.used[c] += padded
        return c, off

    # ---- entries
    def lookup(self, key):
        """-> the key's committed entry, or None"""
        e = self.table.get(key)
        return e if e is not None and e.committed else None

    def note(self, hit):
        """a loader has served an example (or a whole batch) from the cache, or not"""
        if hit:
            self.hits += 1
        else:
            self.misses += 1

    def pending(self, key, owner):
        """-> the entry that `owner` has reserved for the key and not yet committed, or None"""
        e = self.table.get(key)
        return e if e is not None and not e.committed and e.owner is owner else None

    def reserve(self, wanted, owner):
        """wanted: [(key, nbytes)], all or none -> their new entries, or None: a key is taken already, the cache is
        closed or the budget does not hold them all.  After the first refusal for want of room nothing more is
        admitted: first come, first kept."""
        if self.closed or any(k in self.table for k, _ in wanted) or \
                len(set(k for k, _ in wanted)) != len(wanted):
            return None
        made = []
        for key, nbytes in wanted:
            at = self._place(int(nbytes))
            if at is None:
                for e in made:
                    self._give_back(e)
                self.full = True
                return None
            e = Entry(key, at[0], at[1], int(nbytes), owner)
            self.table[key] = e
            made.append(e)
        return made

    def _give_back(self, e):
        del self.table[e.key]
        self.spare.setdefault(e.nbytes, []).append((e.chunk, e.offset))

    def release(self, e):
        """a reservation that will not be filled; a committed entry stays"""
        if not e.committed and self.table.get(e.key) is e:
            self._give_back(e)

    def commit(self, e, ready=None, meta=None):
        e.committed, e.ready, e.meta = True, ready, meta
        self.entries += 1
        self.bytes += e.nbytes

    def counters(self):
        return {'hits': self.hits, 'misses': self.misses, 'entries': self.entries, 'bytes': self.bytes}

    # ---- life
    def attach(self, stage):
        """a stage whose side stream reads or fills entries: close() synchronises it before the chunks go"""
        if stage not in self.stages:
            self.stages.append(stage)

    def close(self):
        if self.closed:
            return
        self.closed = True
        try:
            for stage in self.stages:
                stage.close()
        finally:
            self.stages = []
            self.table.clear()
            self.spare.clear()
            self.chunks, self.sizes, self.used = [], [], []


class HostFrameCache(FrameCache):
    """numpy storage, no GPU."""
    device = None

    def _alloc(self, nbytes):
        return np.empty(nbytes, np.uint8)

    def view(self, e, shape, dtype, offset=0):
        """the entry's bytes from `offset` on as a read-only array"""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        a = self.chunks[e.chunk][e.offset + offset:e.offset + offset + n].view(dtype).reshape(shape)
        a.flags.writeable = False
        return a

    def write(self, e, array, offset=0):
        src = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        self.chunks[e.chunk][e.offset + offset:e.offset + offset + src.size] = src


class DeviceFrameCache(FrameCache):
    """torch uint8 chunks in the memory of `device`."""

    def __init__(self, budget_bytes, device, chunk_bytes=CHUNK_BYTES):
        import torch
        FrameCache.__init__(self, budget_bytes, chunk_bytes)
        self.torch, self.device = torch, device

    def _alloc(self, nbytes):
        """a chunk is allocated on the caller's stream and filled and read on the stages' side streams: whatever the
        caller's stream still does with a block that the allocator hands out again has ended before anyone uses it"""
        chunk = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
        self.torch.cuda.current_stream(self.device).synchronize()
        return chunk

    def address(self, e):
        return self.chunks[e.chunk].data_ptr() + e.offset

    def bytes_of(self, e, offset=0, nbytes=None):
        """the entry's bytes [offset, offset + nbytes) as a uint8 tensor over the chunk"""
        lo = e.offset + offset
        return self.chunks[e.chunk][lo:lo + (e.nbytes - offset if nbytes is None else nbytes)]


def summary_line(cache, train=None, val=None):
    """the run's one line about its cache: the counters, and the loaders' own"""
    c = cache.counters()
    line = 'device cache: hits %d misses %d entries %d bytes %d of %d' % (c['hits'], c['misses'], c['entries'],
                                                                          c['bytes'], cache.budget)
    if train is not None:
        line += '; train hits %d misses %d' % (train.cache_hits, train.cache_misses)
    if val is not None:
        line += '; validation hits %d misses %d (%d after the first pass)' % (
            val.cache_hits, val.cache_misses, val.cache_misses - val.first_pass_misses)
    return line
