"""Streaming FRB-style pipeline (BASELINE.json configs[4]; SURVEY.md §8(d)
config 5): continuous filterbank blocks -> zero-DM -> downsample -> batched DM
sweep, with pinned-host H2D copies overlapped with compute.

Zero-DM modes (bin/zero_dm_filter.py:30-39 subtracts each spectrum's channel
mean; for integer data the mean is rounded half-to-even and the difference is
taken in the data dtype):
  * ``"auto"`` (default): ``"wrap"`` -- the reference's uint8 result --
    where the exact path applies (8-bit input), else ``"float"``.
  * ``"int"`` (8-bit input, downsamp <= 2): x - round(mean) as an
    exact signed integer (the reference's rounding without the uint8 wrap),
    co-added and offset into 16-bit samples <= 1023 (pdd_zdm_int_downsample)
    so the exact packed-u16 sweep runs; the plane bias is removed in the
    sweep epilogue.  Every plane value is an exact integer.
  * ``"wrap"``: the reference's uint8 result, (x - round(mean)) mod 256, on
    the same exact 16-bit path (downsamp <= 4).
  * ``"float"`` (``True``): x - mean in float32, then the float32 sweep
    (the reference's semantics for float data).
  * ``False``: no filter (8-bit input, downsamp <= 4: exact 16-bit path).

Packed input (``nbits`` 1, 2 or 4: chunks are uint8 [n, nchan*nbits/8] in
SIGPROC bit order, and the raw buffers and copies below hold packed rows):
without a mask, on 16-byte packed rows and with the image's bound <= 1023
(``ds vmax`` for no filter, ``2 ds vmax`` for "int", ``255 ds`` for "wrap",
vmax = 2**nbits - 1) the prologue is pdd_zdm_packed_int_downsample, unpack
included; otherwise the block is unpacked (pdd_unpack_bits) into an 8-bit
block that takes the 8-bit path.  ``"auto"`` is then ``"int"`` where its bound
fits, else ``"float"`` (a uint8 wrap of 2-bit values is noise).

PSRFITS input (``decoder``: a formats.psrfits.PsrfitsDecoder): chunks are the
file's own SUBINT rows, uint8 [k, row_bytes] -- the rows of the block's
samples, a seam row in both chunks -- copied into rotating device row
buffers and decoded there (pdd_psrfits_block) into one raw block of the
decoder's type, 8-bit or float32, which takes the paths above; the overlap is
decoded from the next chunk's rows straight to the block's tail
(``StreamingSweep._call_rows``).

Per input chunk (``block`` spectra of the stream, time-major [n, nchan] in
file order, 8/16-bit or float32):

    copy stream : pinned chunk i --H2D--> raw[i % 3][0:ov]      (head, event)
                  pinned chunk i --H2D--> raw[i % 3][ov:n]     (rest, event)
    compute     : raw[(i-1) % 3][block : block + ov] <- raw[i % 3][0 : ov]   (D2D)
                  [injector.apply(raw[(i-1) % 3]): synthetic signals added, in place;
                   chunk i's head is still untouched when it is copied above]
                  [rfimask.apply(raw[(i-1) % 3]): masked cells <- fill, in place]
                  prologue(raw[(i-1) % 3])  -> [C, (block + ov)/ds] u16 (or f32)
                  DMSweep (interleave + sweep, trim)   -> plane [D, block/ds]

``ov = max_bin * ds`` input spectra (the largest dispersion delay of the grid
at the downsampled rate) of chunk i are appended to block i-1, so the
concatenated per-block planes are exactly -- bit for bit -- the plane of the
one-shot ``zero_dm -> downsample -> sweep(trim=True)`` over the whole stream
(zero-DM is per spectrum, downsampling groups stay aligned because
block % ds == 0, and every plane column sees all of its inputs).

Block i-1 waits only for the HEAD of chunk i (its overlap), so the rest of
chunk i's H2D runs on the copy stream while block i-1 is processed; three raw
buffers rotate so the next chunk's copy never waits for the block being
computed.  Events guard every hand-off.  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .sweep import DMSweep

_CODES = {torch.uint8: _lib.U8, torch.int16: _lib.U16, torch.float32: _lib.F32}


_ZDM = {"none": _lib.ZDM_NONE, "int": _lib.ZDM_INT, "wrap": _lib.ZDM_WRAP}


def unpack_bits(packed, nbits, C, out=None, n=None, stream=None):
    """Device unpack (pdd_unpack_bits) of the first ``n`` packed rows of
    ``packed`` ([rows, >= C*nbits/8] uint8, time-major, SIGPROC bit order)
    into the time-major uint8 block ``out[:n]`` ([rows, >= C]; made here when
    None).  Returns out[:n, :C]."""
    assert packed.dtype == torch.uint8 and packed.dim() == 2 and packed.stride(1) == 1
    n = packed.shape[0] if n is None else int(n)
    if out is None:
        out = torch.empty((n, C), dtype=torch.uint8, device=packed.device)
    assert out.dtype == torch.uint8 and out.stride(1) == 1 and out.shape[0] >= n
    assert packed.shape[0] >= n and out.shape[1] >= C and packed.shape[1] * 8 >= C * nbits
    if n:
        call("pdd_unpack_bits", ptr(packed), int(nbits), n, C, packed.stride(0), ptr(out),
             out.stride(0), stream_ptr(stream))
    return out[:n, :C]


def prologue(raw, n, C, ds, mode, img, offset=0, stream=None, nbits=8):
    """zero-DM (``mode``) + downsample by ``ds`` + corner turn of the
    time-major block raw[:n] into the channel-major image ``img``: 16-bit
    offset integers (pdd_zdm_int_downsample; with ``nbits`` 1, 2 or 4
    pdd_zdm_packed_int_downsample on packed rows) when ``img`` is int16,
    float32 (pdd_zdm_downsample) otherwise."""
    if nbits != 8:
        assert img.dtype == torch.int16, "packed rows feed the 16-bit image only"
        call("pdd_zdm_packed_int_downsample", ptr(raw), int(nbits), n, C, raw.stride(0), ds,
             _ZDM[mode], offset, ptr(img), img.stride(0), stream_ptr(stream))
    elif img.dtype == torch.int16:
        call("pdd_zdm_int_downsample", ptr(raw), _lib.U8, n, C, raw.stride(0), ds, _ZDM[mode],
             offset, ptr(img), img.stride(0), stream_ptr(stream))
    else:
        call("pdd_zdm_downsample", ptr(raw), _CODES[raw.dtype], n, C, raw.stride(0), ds,
             int(mode != "none"), ptr(img), img.stride(0), stream_ptr(stream))
    return img


class StreamingSweep(object):
    """``StreamingSweep(dms, freqs, dt)(chunks)`` yields ``(t0, plane)``:
    plane columns t0 .. t0 + plane.shape[1] - 1 of the stream's DM-time plane
    (downsampled time index)."""

    def __init__(self, dms, freqs, dt, block=1 << 18, downsamp=2, zero_dm="auto",
                 dtype=torch.uint8, device="cuda", rfimask=None, nbits=8, decoder=None,
                 injector=None):
        _lib.require_gpu()
        # decoder: a formats.psrfits.PsrfitsDecoder -- chunks are the file's
        # own SUBINT rows (pinned uint8 [k, row_bytes]), decoded on the device
        # into the raw block of the decoder's dtype (see __call__)
        self.decoder = decoder
        if decoder is not None:
            assert nbits == 8, "a decoder emits 8-bit or float32 blocks"
            assert decoder.nchan == len(freqs), "the decoder's channels are not the stream's"
            dtype = decoder.torch_dtype
        # nbits 1, 2 or 4: chunks are packed rows, host uint8 [n, C*nbits/8]
        # (SIGPROC bit order), unpacked on the device
        if nbits not in (1, 2, 4, 8):
            raise ValueError("nbits must be 1, 2, 4 or 8")
        self.nbits = int(nbits)
        self.packed = self.nbits < 8
        # rfimask: a pypulsar_amd.rfi.RFIMask applied in place to every raw
        # block (at its absolute start sample) just before the prologue
        self.rfimask = rfimask
        if rfimask is not None:
            assert rfimask.nchan == len(freqs), "the mask's channels are not the stream's"
            assert dtype in (torch.uint8, torch.float32), "a mask needs 8-bit or float32 input"
        # injector: a pypulsar_amd.inject.Injector applied in place to every
        # raw block (at its absolute start sample) before the mask -- a mask
        # must also excise an injected signal.  Its values depend on (sample,
        # channel) alone, and the overlap rows of a block are copied from the
        # next chunk's head before that chunk is injected, so a row holds the
        # same values in both blocks.  Packed input is unpacked first (never
        # the fused prologue) and clipped to 2^nbits - 1.
        self.injector = injector
        if injector is not None:
            assert injector.C == len(freqs), "the injector's channels are not the stream's"
            assert dtype in (torch.uint8, torch.float32), "injection needs 8-bit or float32 input"
        assert block % downsamp == 0 and 64 % downsamp == 0
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.C = len(self.freqs)
        self.ds = int(downsamp)
        self.dt = dt
        if self.packed:
            assert dtype == torch.uint8, "packed input unpacks to 8-bit values"
            if (self.C * self.nbits) % 8:
                raise ValueError("%d channels of %d bits do not fill whole bytes"
                                 % (self.C, self.nbits))
        self.row_bytes = self.C * self.nbits // 8 if self.packed else self.C
        vmax = (1 << self.nbits) - 1

        def fused_bound(m):
            # bound of the 16-bit image of the fused packed prologue (None:
            # that path does not apply): co-added values for "none", offset
            # ds vmax + co-added (x - round(mean)) for "int", co-added bytes
            # of the uint8 wrap for "wrap"
            if (not self.packed or rfimask is not None or injector is not None
                    or self.row_bytes % 16):
                return None
            return {"none": vmax, "int": 2 * vmax, "wrap": 255}.get(m, 1 << 20) * self.ds

        def exact8(m):
            # the exact 16-bit path of 8-bit blocks: 16-B rows, values <= 1023
            return (dtype == torch.uint8 and m != "float" and self.C % 16 == 0
                    and self.ds <= (2 if m == "int" else 4))

        mode = {True: "float", False: "none"}.get(zero_dm, zero_dm)
        if mode == "auto" and self.packed:
            # no reference semantics for packed data (a uint8 wrap of 2-bit
            # values is noise): the exact integer filter where its bound fits
            fbi = fused_bound("int")
            mode = "int" if (fbi is not None and fbi <= 1023) or exact8("int") else "float"
        elif mode == "auto":
            # the reference's own result for 8-bit data: uint8 wrap
            # (zero_dm_filter.py:30-39), exact on the 16-bit path
            mode = "wrap" if (dtype == torch.uint8 and self.C % 16 == 0 and self.ds <= 4) else "float"
        if mode not in ("int", "wrap", "float", "none"):
            raise ValueError("zero_dm must be 'auto', 'int', 'wrap', 'float', True or False")
        self.dtype = dtype
        self.device = torch.device(device)
        # packed input, fused path: pdd_zdm_packed_int_downsample -> the u16
        # sweep (no mask, 16-B packed rows, values <= 1023); otherwise packed
        # blocks are unpacked (pdd_unpack_bits) and take the 8-bit path below
        fb = fused_bound(mode)
        self.fused = fb is not None and fb <= 1023
        # the exact 16-bit path: 8-bit input, 16-B rows, co-added values <= 1023
        self.exact = self.fused or exact8(mode)
        if mode in ("int", "wrap") and not self.exact:
            if self.packed:
                raise ValueError("zero_dm=%r on %d-bit input needs values <= 1023 on 16-byte "
                                 "packed rows without a mask, or the 8-bit path's nchan %% 16 "
                                 "== 0 and downsamp <= %d" % (mode, self.nbits,
                                                              2 if mode == "int" else 4))
            raise ValueError("zero_dm=%r needs 8-bit input, nchan %% 16 == 0 and downsamp <= %d"
                             % (mode, 2 if mode == "int" else 4))
        self.mode = mode
        self.zero_dm = mode != "none"
        if self.fused:
            self.offset = vmax * self.ds if mode == "int" else 0
            self.input_max = fb
        else:
            self.offset = 255 * self.ds if mode == "int" else 0
            # bound of the 16-bit image: offset + co-added (x - round(mean)) for
            # "int" (<= 510 ds), co-added bytes for "wrap" / "none" (<= 255 ds)
            self.input_max = (510 if mode == "int" else 255) * self.ds if self.exact else None
        self.sweep = DMSweep(dms, self.freqs, dt * self.ds, dtype="u16" if self.exact else "f32",
                             input_max=self.input_max)
        self.D = self.sweep.D
        self.max_bin = max(0, self.sweep.max_bin)
        self.block = int(block)
        self.ov = self.max_bin * self.ds
        assert self.ov <= self.block, "block must hold the overlap (max delay x downsamp)"
        n_raw = self.block + self.ov
        self.nbuf = 3
        # with a decoder the row buffers rotate and one raw block suffices: it
        # is written (decode) and read (prologue) on the compute stream alone
        self.raw = [torch.empty((n_raw, self.row_bytes), dtype=dtype, device=self.device)
                    for _ in range(self.nbuf if decoder is None else 1)]
        self.rows = None
        if decoder is not None:
            self.rows = [torch.empty((decoder.max_rows(self.block), decoder.row_bytes),
                                     dtype=torch.uint8, device=self.device)
                         for _ in range(self.nbuf)]
        # the 8-bit block of a packed stream off the fused path
        self.unpacked = (torch.empty((n_raw, self.C), dtype=torch.uint8, device=self.device)
                         if self.packed and not self.fused else None)
        self.img = torch.empty((self.C, n_raw // self.ds),
                               dtype=torch.int16 if self.exact else torch.float32,
                               device=self.device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.h2d_head = [torch.cuda.Event() for _ in range(self.nbuf)]
        self.h2d = [torch.cuda.Event() for _ in range(self.nbuf)]
        self.free = [torch.cuda.Event() for _ in range(self.nbuf)]
        for e in self.free:
            e.record(torch.cuda.current_stream(self.device))

    @property
    def n_out_block(self):
        return self.block // self.ds

    def _process(self, raw, n_valid, out=None, s0=0):
        """zero-DM + downsample + sweep of raw[:n_valid] -> plane (trim=True);
        s0: the block's first input sample (for the injector and the RFI mask)."""
        if self.unpacked is not None:
            unpack_bits(raw, self.nbits, self.C, self.unpacked, n_valid)
            raw = self.unpacked
        if self.injector is not None:
            self.injector.apply(raw[:n_valid], s0,
                                vmax=(1 << self.nbits) - 1 if self.packed else None)
        if self.rfimask is not None:
            self.rfimask.apply(raw[:n_valid], s0)
        nd = n_valid // self.ds
        n_out = max(0, nd - self.max_bin)
        if out is None:
            out = torch.empty((self.D, max(n_out, 0)), dtype=torch.float32, device=self.device)
        if n_out == 0:
            return out[:, :0]
        prologue(raw, n_valid, self.C, self.ds, self.mode, self.img, self.offset,
                 nbits=self.nbits if self.fused else 8)
        self.sweep(self.img[:, :nd], trim=True, out=out, out_bias=-float(self.offset * self.C))
        return out[:, :n_out]

    def __call__(self, chunks, planes=None, start_block=0):
        """chunks: iterable of host tensors [n, C] (packed input: uint8
        [n, C*nbits/8]; pinned for an asynchronous
        copy; every chunk but the last must hold exactly ``block`` spectra).
        planes: optional list of preallocated [D, block/ds] device planes,
        used in rotation by EMITTED-block count (block j -> planes[j % len]),
        so a consumer holding the last len(planes) - 1 planes never sees them
        overwritten.  Yields (t0, plane).

        Restart by block index: a block's plane depends only on its own chunk
        and the head of the next one, so a run resumed at block k -- chunks
        k, k+1, ... of the stream and ``start_block=k`` -- yields exactly the
        (t0, plane) pairs of blocks k, k+1, ... of the uninterrupted run."""
        if self.decoder is not None:
            for item in self._call_rows(chunks, planes, start_block):
                yield item
            return
        cur = torch.cuda.current_stream(self.device)
        prev = None  # (buffer index, n spectra)
        t0 = int(start_block) * self.n_out_block
        s0 = int(start_block) * self.block  # first input sample of the block in `prev`
        i = -1
        emitted = 0
        for i, chunk in enumerate(chunks):
            b = i % self.nbuf
            n = chunk.shape[0]
            assert chunk.shape[1] == self.row_bytes and n <= self.block
            head = min(self.ov, n)
            self.copy_stream.wait_event(self.free[b])
            with torch.cuda.stream(self.copy_stream):
                if head:
                    self.raw[b][:head].copy_(chunk[:head], non_blocking=True)
                self.h2d_head[b].record(self.copy_stream)
                if n > head:
                    self.raw[b][head:n].copy_(chunk[head:], non_blocking=True)
            self.h2d[b].record(self.copy_stream)
            if prev is not None:
                pb, pn = prev
                assert pn == self.block, "only the last chunk may be short"
                cur.wait_event(self.h2d[pb])       # the block's own chunk
                cur.wait_event(self.h2d_head[b])   # the next chunk's first ov spectra
                if head:
                    self.raw[pb][pn:pn + head].copy_(self.raw[b][:head])
                out = None if planes is None else planes[emitted % len(planes)]
                emitted += 1
                plane = self._process(self.raw[pb], pn + head, out, s0)
                self.free[pb].record(cur)
                yield t0, plane
                t0 += plane.shape[1]
                s0 += pn
            prev = (b, n)
        if prev is not None:
            pb, pn = prev
            cur.wait_event(self.h2d[pb])
            out = None if planes is None else planes[emitted % len(planes)]
            plane = self._process(self.raw[pb], pn, out, s0)
            self.free[pb].record(cur)
            yield t0, plane

    def _call_rows(self, chunks, planes, start_block):
        """__call__ with a decoder.  Chunk i (counted from ``start_block``) is
        a host uint8 [k, row_bytes] tensor (pinned for an asynchronous copy)
        holding the SUBINT rows of samples [i block, (i+1) block) as
        ``decoder.rows_for`` names them; a row on a block seam is in both
        chunks.

            copy stream : chunk i's rows holding its first ov samples
                              --H2D--> rows[i % 3]             (head, event)
                          its other rows --H2D--> rows[i % 3]  (rest, event)
            compute     : decode(rows[(i-1) % 3]) -> raw[0 : block]
                          decode(rows[i % 3], first ov samples) -> raw[block : block + ov]
                          [mask], prologue, sweep as without a decoder

        The decode addresses any sample range of the rows, so the overlap is
        decoded where it is needed (no D2D append); ``free[b]`` guards the row
        buffer."""
        dec = self.decoder
        cur = torch.cuda.current_stream(self.device)
        raw = self.raw[0]
        prev = None  # (buffer index, n spectra, rows, offset of the first sample)
        t0 = int(start_block) * self.n_out_block
        s0 = int(start_block) * self.block
        emitted = 0
        for i, chunk in enumerate(chunks):
            b = i % self.nbuf
            start = (int(start_block) + i) * self.block
            row0, nrows, off = dec.rows_for(start, self.block)
            n = min(self.block, dec.number_of_samples - start)
            assert n > 0 and tuple(chunk.shape) == (nrows, dec.row_bytes), \
                "chunk %d must hold the %d rows of its samples" % (i, nrows)
            head = min(self.ov, n)
            nh = (off + head - 1) // dec.nsblk + 1 if head else 0  # rows of the head
            self.copy_stream.wait_event(self.free[b])
            with torch.cuda.stream(self.copy_stream):
                if nh:
                    self.rows[b][:nh].copy_(chunk[:nh], non_blocking=True)
                self.h2d_head[b].record(self.copy_stream)
                if nrows > nh:
                    self.rows[b][nh:nrows].copy_(chunk[nh:], non_blocking=True)
            self.h2d[b].record(self.copy_stream)
            if prev is not None:
                pb, pn, pr, poff = prev
                assert pn == self.block, "only the last chunk may be short"
                cur.wait_event(self.h2d[pb])
                cur.wait_event(self.h2d_head[b])
                dec.decode(self.rows[pb], pr, poff, pn, raw)
                if head:
                    dec.decode(self.rows[b], nh, off, head, raw[pn:])
                out = None if planes is None else planes[emitted % len(planes)]
                emitted += 1
                plane = self._process(raw, pn + head, out, s0)
                self.free[pb].record(cur)
                yield t0, plane
                t0 += plane.shape[1]
                s0 += pn
            prev = (b, n, nrows, off)
        if prev is not None:
            pb, pn, pr, poff = prev
            cur.wait_event(self.h2d[pb])
            dec.decode(self.rows[pb], pr, poff, pn, raw)
            out = None if planes is None else planes[emitted % len(planes)]
            plane = self._process(raw, pn, out, s0)
            self.free[pb].record(cur)
            yield t0, plane

    def close(self):
        self.sweep.close()
