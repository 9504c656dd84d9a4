"""The buffer ring under the device encoders (png.DeviceEncoder, jpeg.DeviceEncoder and, through the latter,
figure.DeviceFigures): what a batch loop needs to get variable-length payloads made on the device into files while the
device is on the next batch.  The encoders add the bound, the one engine call and the framing.
"""


class Ring(object):
    """Two buffer sets, each the device payload buffer (`batch` rows of `bound` bytes, rounded up to 16), `meta_rows`
    rows of int32 per image (row 0: the payload's length) with their pinned copy, a pinned payload buffer and whatever
    a subclass declares; allocated once for batches of at most `batch` images.  Per batch, in this order:

      slot = encode(src)      on the current stream: launch(slot, src, n) for the n images of src, then the meta rows
                              into pinned memory.  Nothing waits.
      fetch(slot)             once the host knows that stream got past encode(): the download of the USED bytes only,
                              on the ring's own stream (it does not queue behind the caller's next batch).
      file_bytes(slot, j)     any thread: waits for that download, -> frame(slot, j, payload), the bytes of image j's file.

    A set is reused by the batch after next: encode() makes the device wait for the set's last download, and the
    caller must be through with file_bytes() of a set before it calls fetch() on it again.  The pinned payload buffer
    holds the batch's payloads one after the other at 16-byte offsets; it starts at `pinned_bytes`, and fetch()
    replaces it by a larger one if a batch ever needs that."""

    def __init__(self, engine, batch, bound, meta_rows, pinned_bytes):
        import torch
        self.eng, self.batch = engine, max(int(batch), 1)
        stride = (int(bound) + 15) // 16 * 16
        self.slots = [dict(out=torch.empty((self.batch, stride), dtype=torch.uint8, device=engine.device),
                           meta=torch.empty((meta_rows, self.batch), dtype=torch.int32, device=engine.device),
                           out_h=torch.empty((int(pinned_bytes),), dtype=torch.uint8).pin_memory(),
                           meta_h=torch.empty((meta_rows, self.batch), dtype=torch.int32).pin_memory(), copied=None, n=0)
                      for _ in range(2)]
        self.stream = torch.cuda.Stream(device=engine.device)
        self.count = 0
        self.downloaded = 0                 # payload bytes fetched so far

    def declare(self, name, shape, dtype):
        """one more device buffer per set: slot[name]"""
        import torch
        for slot in self.slots:
            slot[name] = torch.empty(shape, dtype=dtype, device=self.eng.device)

    def next_slot(self):
        """the set the next encode() uses"""
        return self.slots[self.count % 2]

    def encode(self, src):
        import torch
        slot = self.next_slot()
        self.count += 1
        n = slot['n'] = int(src.shape[0])
        if slot['copied'] is not None:
            torch.cuda.current_stream(self.eng.device).wait_event(slot['copied'])
        self.launch(slot, src, n)
        slot['meta_h'].copy_(slot['meta'], non_blocking=True)
        return slot

    def fetch(self, slot):
        import torch
        # host copies: the set's next encode() overwrites meta_h while file_bytes() of this batch may still run
        slot['rows'] = [[int(v) for v in row[:slot['n']]] for row in slot['meta_h'].numpy()]
        lengths, starts = slot['rows'][0], [0]
        for nb in lengths:
            starts.append(starts[-1] + (nb + 15) // 16 * 16)
        slot['starts'] = starts
        if starts[-1] > slot['out_h'].numel():
            slot['out_h'] = torch.empty((starts[-1],), dtype=torch.uint8).pin_memory()
        with torch.cuda.stream(self.stream):
            for j, nb in enumerate(lengths):
                slot['out_h'][starts[j]:starts[j] + nb].copy_(slot['out'][j, :nb], non_blocking=True)
                self.downloaded += nb
            slot['copied'] = torch.cuda.Event()
            slot['copied'].record(self.stream)

    def file_bytes(self, slot, j):
        slot['copied'].synchronize()
        lo = slot['starts'][j]
        return self.frame(slot, j, slot['out_h'][lo:lo + slot['rows'][0][j]].numpy().tobytes())
