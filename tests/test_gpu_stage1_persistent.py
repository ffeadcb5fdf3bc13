"""The persistent, prefetching stage 1 of the factorised sweep (pdd_sweep.hip
k_fx_stage1_p) and the time-major input layout (pdd_sweep_execute_tm).

Every plane here must be BIT-IDENTICAL to the channel-by-channel sweep
(factor=False) of the same input, pads and trim, and sampled rows to the
independent fused single-DM kernel (Spectra.dedispersed_series); the pattern
image is poisoned before every stage 1 (pdd_sweep_plan_set_poison), so an
element stage 1 skipped and stage 2 read shows.  The shapes give stage 1 more
(group, element block) items than the device holds persistent workgroups
(at most 5 per CU of 256: 1280), so the persistent kernel runs; the smallest
case stays on the one-item kernel."""
import numpy as np
import pytest

from conftest import band

DT = 64e-6
_CACHE = {}


@pytest.fixture(autouse=True)
def poison_patterns(monkeypatch):
    from pypulsar_amd import sweep
    monkeypatch.setitem(sweep.TEST_SWITCHES, "poison", True)


def block(C, N, kind="u8", seed=5):
    """[C, N] device block of the given kind (cached: the tests share it)."""
    import torch
    key = (C, N, kind, seed)
    if key not in _CACHE:
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + C)
        hi = 256 if kind == "u8" else 1024
        x = torch.randint(0, hi, (C, N), generator=g, device="cuda", dtype=torch.int16)
        _CACHE[key] = {"u8": lambda: x.to(torch.uint8), "u16": lambda: x,
                       "f32": lambda: x.float()}[kind]()
    return _CACHE[key]


def reference(dms, freqs, x, code, pad=0, trim=True, key=None):
    """The channel-by-channel plane (cached under ``key``)."""
    from pypulsar_amd.sweep import DMSweep
    if key is not None and key in _CACHE:
        return _CACHE[key]
    plain = DMSweep(dms, freqs, DT, dtype=code, factor=False)
    ref = plain(x, padval=pad, trim=trim)
    assert plain.factor_info({"u8": 1, "u16": 2, "f32": 0}[code])[0] == 0
    plain.close()
    if key is not None:
        _CACHE[key] = ref
    return ref


def dm_grid(freqs, D, max_bin):
    """D trials from DM 0 up to the DM whose largest delay is ~max_bin samples."""
    k = 4.148808e3 * abs(freqs.min() ** -2 - freqs.max() ** -2) / DT
    return np.linspace(0.0, max_bin / k, D)


@pytest.mark.gpu
@pytest.mark.parametrize("C,g,logN,D,mb", [
    (264, 4, 17, 48, 600),    # 66 groups x 33 blocks
    (260, 4, 17, 200, 600),   # 65 groups: an odd count
    (264, 2, 16, 48, 600),    # 132 groups of 2 x 17 blocks
    (68, 4, 19, 48, 300),     # 17 groups (< 8 per XCD share, not a multiple of 8) x 129 blocks
    (264, 4, 18, 64, 600),    # 66 x 65 = 4290 items: every workgroup walks >= 3
    (64, 4, 14, 48, 300),     # 16 x 5 items: fewer than one wave of workgroups, the one-item kernel
])
def test_groups_and_walk_length(gpu, C, g, logN, D, mb):
    import torch
    from pypulsar_amd.formats.spectra import Spectra
    from pypulsar_amd.sweep import DMSweep
    N = 1 << logN
    freqs = band(C)
    dms = dm_grid(freqs, D, mb)
    x = block(C, N)
    fx = DMSweep(dms, freqs, DT, dtype="u8", factor="force%d" % g)
    assert fx.factor_info()[0] == g and fx.direct_stage1()
    assert mb - 10 <= fx.max_bin <= mb + 10
    got = fx(x)
    fx.close()
    assert torch.equal(got, reference(dms, freqs, x, "u8"))
    s = Spectra._from_device(freqs, DT, x.float())
    for d in (0, 1, D // 2, D - 1):
        ser = s.dedispersed_series(dms[d], padval=0, trim=True)[:got.shape[1]]
        assert torch.equal(ser, got[d]), "row %d != dedispersed_series" % d


@pytest.mark.gpu
@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("g", [4, 2])
def test_pads_trim_band_orders(gpu, descending, g):
    import torch
    from pypulsar_amd.sweep import DMSweep
    C, N, D = 264, 1 << 17, 48
    freqs = band(C, descending=descending)
    dms = dm_grid(freqs, D, 500)
    x = block(C, N)
    fx = DMSweep(dms, freqs, DT, dtype="u8", factor="force%d" % g)
    assert fx.factor_info()[0] == g
    for pad in (0, 7, "rotate"):
        for trim in (True, False):
            ref = reference(dms, freqs, x, "u8", pad, trim, key=("ptb", descending, pad, trim))
            assert torch.equal(fx(x, padval=pad, trim=trim), ref), (pad, trim)
    fx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,code", [("u16", 2), ("f32", 0)])
@pytest.mark.parametrize("g", [4, 2])
def test_input_types(gpu, kind, code, g):
    """16-bit samples <= 1023 (packed elements held in registers) and float32
    input (1024-element blocks; integer-valued, so the regrouped float sum is
    exact)."""
    import torch
    from pypulsar_amd.sweep import DMSweep
    C, N, D = 264, 1 << 17, 200
    freqs = band(C)
    dms = dm_grid(freqs, D, 500)
    x = block(C, N, kind)
    fx = DMSweep(dms, freqs, DT, dtype=kind, factor="force%d" % g)
    assert fx.factor_info(code)[0] == g and fx.direct_stage1(code)
    for pad, trim in ((0, True), ("rotate", False)):
        ref = reference(dms, freqs, x, kind, pad, trim, key=("types", kind, pad, trim))
        assert torch.equal(fx(x, padval=pad, trim=trim), ref), (pad, trim)
    fx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("g", [4, 2])
def test_layouts_agree(gpu, g):
    """Channel-major rows with ld > N (a multiple of 4: dword loads; odd: the
    byte path), pieces of 2^10 samples from a non-zero column offset,
    time-major spectra with ld_t > C, and time-major spectra one byte off
    16-byte alignment (the generic accessor): one plane."""
    import torch
    from pypulsar_amd.sweep import DMSweep
    C, N, D = 264, 1 << 17, 48
    freqs = band(C)
    dms = dm_grid(freqs, D, 500)
    x = block(C, N)
    ref = reference(dms, freqs, x, "u8", key=("layouts",))
    fx = DMSweep(dms, freqs, DT, dtype="u8", factor="force%d" % g)
    n_out = fx.n_out(N)
    for extra in (24, 3):
        wide = torch.zeros((C, N + extra), dtype=torch.uint8, device="cuda")
        wide[:, :N] = x
        assert torch.equal(fx(wide[:, :N]), ref), "ld = N + %d" % extra
    x_off, n_cols = 1000, n_out - 1500
    want = ref[:, x_off:x_off + n_cols]
    out = torch.empty((D, n_cols), dtype=torch.float32, device="cuda")
    P = 1 << 10
    xp = x.view(C, N // P, P).permute(1, 0, 2).contiguous()
    assert torch.equal(fx.sweep_pieces(xp, N, P, x_off, n_cols, out), want), "pieces"
    # time-major, ld_t = C + 8, then ld_t = C at offset 0 and at offset 1 element
    tm = torch.zeros((N, C + 8), dtype=torch.uint8, device="cuda")
    tm[:, :C] = x.t()
    out.fill_(-1.0)
    assert torch.equal(fx.sweep_timemajor(tm[:, :C], N, x_off, n_cols, out), want), "ld_t > C"
    flat = torch.zeros(N * C + 16, dtype=torch.uint8, device="cuda")
    for o in (0, 1):
        v = flat[o:o + N * C].view(N, C)
        v.copy_(x.t())
        assert v.data_ptr() % 16 == o
        out.fill_(-1.0)
        assert torch.equal(fx.sweep_timemajor(v, N, x_off, n_cols, out), want), "offset %d" % o
    full = torch.empty((D, n_out), dtype=torch.float32, device="cuda")
    assert torch.equal(fx.sweep_timemajor(tm[:, :C], N, 0, n_out, full), ref)
    fx.close()


@pytest.mark.gpu
def test_timemajor_other_plans(gpu):
    """Time-major input through the generic accessor: a channel-by-channel
    plan (the interleave pre-pass) and float32 input."""
    import torch
    from pypulsar_amd.sweep import DMSweep
    C, N, D = 264, 1 << 16, 200
    freqs = band(C)
    dms = dm_grid(freqs, D, 500)
    for kind, factor in (("u8", False), ("f32", "force4")):
        x = block(C, N, kind)
        ref = reference(dms, freqs, x, kind)
        sw = DMSweep(dms, freqs, DT, dtype=kind, factor=factor)
        out = torch.empty_like(ref)
        assert torch.equal(sw.sweep_timemajor(x.t().contiguous(), N, 0, ref.shape[1], out), ref), kind
        sw.close()


@pytest.mark.gpu
def test_segments(gpu):
    """Several segments (pdd_sweep_plan_set_segment_bytes), each its own stage
    1, from channel-major and from time-major input."""
    import torch
    from pypulsar_amd.sweep import DMSweep
    C, N, D = 264, 1 << 18, 48
    freqs = band(C)
    dms = dm_grid(freqs, D, 500)
    x = block(C, N)
    ref = reference(dms, freqs, x, "u8", key=("segments",))
    fx = DMSweep(dms, freqs, DT, dtype="u8", factor="force4")
    n_pat = fx.factor_info()[1]
    # rows x (delay span + ~12000 elements of eighths): three segments of N
    fx.set_segment_bytes((C + n_pat + 2) * 16 * (fx.max_bin + 64 + 12000))
    assert torch.equal(fx(x), ref)
    out = torch.empty_like(ref)
    assert torch.equal(fx.sweep_timemajor(x.t().contiguous(), N, 0, ref.shape[1], out), ref)
    fx.close()


@pytest.mark.gpu
def test_unread_blocks_are_skipped(gpu):
    """Plane-aligned tiles, delays up to ~2000 samples: the pattern rows are
    Qs + ~2000 elements long, and the trials of a high-frequency group (base
    shifts near 0) read none of a row's last blocks.  From the delay table a
    group's rows are read inside [min base shift, Qs + max base shift) (+ 320
    elements of slack either side: a time tile, DMA granules); the 512-element blocks that
    range touches, summed over the patterns, are fewer bytes than
    pattern_bytes() -- whole blocks are unread -- and stage 1 alone, run into
    a poisoned buffer, must leave at least the difference untouched, while
    the plane (stage 2 over the same buffer) still equals the reference."""
    import torch
    from oracle import spectra_oracle as orc
    from pypulsar_amd.sweep import DMSweep
    C, N, D, g = 264, 1 << 17, 200, 4
    freqs = band(C)
    dms = dm_grid(freqs, D, 2000)
    x = block(C, N)
    ref = reference(dms, freqs, x, "u8", key=("skip",))
    fx = DMSweep(dms, freqs, DT, dtype="u8", factor="force4", skew=False)
    n_pat = fx.factor_info()[1]
    n_out = fx.n_out(N)
    nbytes = fx.pattern_bytes(n_out)
    nR = nbytes // 16 // (n_pat + 1)
    assert nbytes == (n_pat + 1) * nR * 16
    Qs = -(-n_out // 8 // 128) * 128
    tab = orc.sweep_table(dms, freqs, DT)
    blocks = -(-nR // 512)
    implied, slack, pats_all = 0, 320, 0
    for c0 in range(0, C, g):
        rel = tab[:, c0:c0 + g] - tab[:, c0:c0 + 1]
        pats = len(np.unique(rel, axis=0))
        lo = max(0, int(tab[:, c0].min()) - slack)
        hi = min(nR, Qs + int(tab[:, c0].max()) + slack)
        implied += pats * (-(-hi // 512) - lo // 512)
        pats_all += pats
    assert pats_all == n_pat
    assert implied * 512 * 16 < nbytes - nR * 16 - n_pat * 512 * 16, "no whole block unread"
    pbuf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((D, n_out), dtype=torch.float32, device="cuda")
    fx.sweep_pieces_stage(x, N, 0, 0, n_out, None, pbuf, 1)
    img = pbuf.view(n_pat + 1, nR, 16)[:n_pat]
    written = (img != 255).any(dim=2)                       # [n_pat, nR] elements stage 1 wrote
    padded = torch.zeros((n_pat, blocks * 512), dtype=torch.bool, device="cuda")
    padded[:, :nR] = written
    touched = int(padded.view(n_pat, blocks, 512).any(dim=2).sum())
    assert 0 < touched <= implied, (touched, implied, n_pat * blocks)
    fx.sweep_pieces_stage(x, N, 0, 0, n_out, out, pbuf, 2)
    assert torch.equal(out, ref)
    fx.close()


@pytest.mark.gpu
def test_sharded_one_rank_sweeps_file_order(gpu):
    """DMShardedSweep(world 1, 4 batches) at 2^16 spectra: the batches are
    swept from the time-major part itself (no channel-major block), as one
    call and as the exchange_batch / sweep_batch loop of the bench's PCIe
    leg; both equal the one-shot plane."""
    import torch
    from pypulsar_amd.sharding import DMShardedSweep
    C, N, D, NB = 264, 1 << 16, 48, 4
    freqs = band(C)
    dms = dm_grid(freqs, D, 500)
    x = block(C, N)
    ref = reference(dms, freqs, x, "u8", key=("sharded",))
    part = x.t().contiguous().view(NB, N // NB, C)
    ds = DMShardedSweep(dms, freqs, DT, N, dtype=torch.uint8, n_batches=NB, device="cuda",
                        factor="force4")
    assert ds.sw.direct_stage1()
    planes = ds(part)
    assert torch.equal(torch.cat(list(planes), dim=1), ref)
    if ds.tm:
        assert ds.x is None and ds.cm == []
    for p in ds.planes:
        p.fill_(-1.0)
    for k in range(NB):
        assert ds.exchange_batch(part, k) is None
        assert ds.sweep_batch(k) == []
    assert torch.equal(ds.plane(), ref)
    ds.close()
