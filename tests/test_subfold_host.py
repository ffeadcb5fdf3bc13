"""Host side of the subband fold (pypulsar_amd/subfold.py): its brute-force
restatement (tests/subfold_oracle.py) pinned to the oracles that are pinned
already (the sweep's and the fold's), the ladder arithmetic, the candidate
conversion, the block planning, the .npz round trip and the limit checks.
No GPU."""
import numpy as np
import pytest

import fold_oracle as fo
import subfold_oracle as so
from conftest import band, u8_data
from oracle import spectra_oracle as orc

DT = 64e-6


@pytest.mark.parametrize("descending", [True, False])
@pytest.mark.parametrize("dm", [0.0, 3.0, 60.0, 400.0])
def test_oracle_against_sweep_and_fold_oracles(descending, dm):
    C, N, npart, nsub, nbins = 32, 6001, 5, 8, 24
    freqs = band(C, descending)
    x = u8_data(C, N, 7 + int(dm))                      # [C, N]
    jobs = [(dm, 1.0 / (37.3 * DT), 0.0, 0.0), (dm, 91.3, 3.0e4, 0.4)]
    cube, cnt, chansum, chansq = so.subfold(x.T, freqs, DT, jobs, npart, nsub, nbins)
    table = orc.sweep_table([dm], freqs, DT)
    bmax = int(table.max())
    row = orc.sweep_plane(x.astype(np.float64), table)[:, :N - bmax]
    assert row.shape == (1, N - bmax)
    prof, pc, _ = fo.fold_rows(row, [(0,) + fo.phase_steps(f, fd, DT, p0) for _, f, fd, p0 in jobs],
                               npart, nbins)
    np.testing.assert_array_equal(cube.sum(axis=2), prof)
    np.testing.assert_array_equal(cnt, pc)
    b, _ = so.delays_of(dm, freqs, DT)
    nf = so.geometry(N, bmax, npart)[2]
    assert nf == npart * ((N - bmax) // npart) and cnt[0].sum() == nf
    xi = x.astype(np.int64)
    for c in range(C):
        seg = xi[c, b[c]:b[c] + nf]
        assert chansum[0, c] == seg.sum() and chansq[0, c] == (seg * seg).sum()
    np.testing.assert_array_equal(chansum[0], chansum[1])
    # the module's host geometry is the oracle's
    from pypulsar_amd.subfold import Jobs
    jb = Jobs(freqs, DT, npart, N, [dm], [jobs[0][1]])
    np.testing.assert_array_equal(jb.table[0], b)
    assert (jb.bmax[0], jb.L[0], jb.nfold[0]) == (bmax, (N - bmax) // npart, nf)
    # subbands partition the channels: a finer split sums to a coarser one
    c16 = so.subfold(x.T, freqs, DT, jobs[:1], npart, 16, nbins)[0]
    np.testing.assert_array_equal(c16.reshape(1, npart, 8, 2, nbins).sum(axis=3), cube[:1])


@pytest.mark.parametrize("descending", [True, False])
def test_ladder_and_shifts(descending):
    from pypulsar_amd import subfold as sf
    from pypulsar_amd.delays import delay_from_DM, subband_layout
    freqs = band(64, descending)
    nsub, nbins, dm, f = 8, 64, 55.0, 1.0 / 0.05003
    u = sf.subband_u(freqs, nsub)
    np.testing.assert_array_equal(u, so.subband_u(freqs, nsub))
    ctr = subband_layout(freqs, nsub)[2]
    np.testing.assert_array_equal(u, delay_from_DM(1.0, ctr) - delay_from_DM(1.0, freqs.max()))
    assert np.all(u > 0)
    dms = sf.default_ladder(dm, f, freqs, nsub, nbins)
    np.testing.assert_array_equal(dms, so.default_ladder(dm, f, freqs, nsub, nbins))
    assert len(dms) == nbins + 1 and dms[nbins // 2] == dm
    ddm = sf.ladder_step(f, freqs, nsub, nbins)
    np.testing.assert_allclose(np.diff(dms), ddm, rtol=1e-12)
    # one step moves the lowest subband by one bin, the ladder spans half a turn each way
    r = sf.ladder_shifts(dm, f, dms, freqs, nsub, nbins)
    assert r.dtype == np.int32 and r.shape == (nbins + 1, nsub)
    np.testing.assert_array_equal(r, so.ladder_shifts(dm, f, dms, freqs, nsub, nbins))
    low = int(np.argmax(u))
    assert np.all(r[nbins // 2] == 0) and r[nbins // 2 + 1, low] == 1
    assert r[nbins // 2 - 1, low] == nbins - 1 and r[-1, low] == nbins // 2
    assert r.min() >= 0 and r.max() < nbins
    # other ladders: one entry, many entries, entries far away (mod nbins)
    for lad in ([dm], np.linspace(0.0, 300.0, 1024), [dm - 1e4, dm + 1e4]):
        got = sf.ladder_shifts(dm, f, lad, freqs, nsub, 50)
        np.testing.assert_array_equal(got, so.ladder_shifts(dm, f, lad, freqs, nsub, 50))
        assert got.min() >= 0 and got.max() < 50
    assert len(sf.default_ladder(dm, f, freqs, nsub, nbins, 7)) == 7


def test_limits_raise():
    from pypulsar_amd import subfold as sf
    freqs = band(64)
    ok = dict(npart=8, nsub=8, nbins=64, ndm=None)
    sf.SubbandFolder(freqs, DT, **ok)
    sf.SubbandFolder(freqs, DT, npart=32, nsub=32, nbins=256, ndm=1024)
    sf.SubbandFolder(freqs, DT, npart=128, nsub=64, nbins=64)
    for bad in (dict(nbins=1), dict(nbins=257), dict(npart=0), dict(npart=129),
                dict(npart=64, nbins=256), dict(nsub=64, nbins=256), dict(nsub=7), dict(nsub=0),
                dict(ndm=0), dict(ndm=1025)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            sf.SubbandFolder(freqs, DT, **kw)
    folder = sf.SubbandFolder(freqs, DT, **ok)
    with pytest.raises(ValueError):
        folder.plan(50000, [-1.0], [10.0])              # negative DM
    with pytest.raises(ValueError):
        folder.plan(100, [60.0], [10.0])                # fewer samples than delays + parts
    with pytest.raises(OverflowError):
        sf.Jobs(freqs, 1e-9, 8, 1 << 40, [1e9], [10.0])  # table entries beyond int32
    jobs = folder.plan(50000, [60.0, 0.0], [10.0, 20.0], 0.0, [0.0, 0.5])
    t = orc.sweep_table([60.0, 0.0], freqs, DT)
    np.testing.assert_array_equal(jobs.table, t)
    assert jobs.table.dtype == np.int32 and jobs.table.min() >= 0
    assert list(jobs.bmax) == [t[0].max(), 0]
    assert list(jobs.L) == [(50000 - t[0].max()) // 8, 50000 // 8]
    for j, (f, p0) in enumerate(((10.0, 0.0), (20.0, 0.5))):
        assert tuple(int(v) for v in jobs.words[j].view(np.uint64)) == fo.phase_steps(f, 0.0, DT, p0)
    with pytest.raises(ValueError):
        folder.ladders(jobs, np.zeros((2, 1025)))
    with pytest.raises(ValueError):
        folder.ladders(jobs, np.zeros((3, 5)))


def test_candidate_conversion():
    from pypulsar_amd.fold import FoldedCandidate
    from pypulsar_amd.periodicity import SiftedCandidate
    from pypulsar_amd.subfold import candidate_params
    N = 100000
    fc = FoldedCandidate(dm=61.5, f=19.98, fd=-1e-3, trial=(3, -2), f_fold=20.0)
    plain = SiftedCandidate(60.0, 265.2, 0.05, 4, 30.0, 9.0)
    acc = SiftedCandidate(33.0, 100.0, 0.01, 2, 20.0, 7.0)
    acc.fd = 0.25
    got = candidate_params([fc, plain, acc, (12.0, 5.0, 0.5), (13.0, 6.0)], N, DT)
    assert got[0] == (61.5, 19.98, -1e-3, (0, 0))        # refined already: trial (0, 0)
    assert got[1] == (60.0, plain.freq, 0.0, (0, 0))
    assert got[2] == (33.0, acc.freq - 0.5 * 0.25 * N * DT, 0.25, (0, 0))
    assert got[3] == (12.0, 5.0, 0.5, (0, 0)) and got[4] == (13.0, 6.0, 0.0, (0, 0))
    assert candidate_params([], N, DT) == []


@pytest.mark.parametrize("max_rows", [1000, 4097, 100000])
def test_block_planning(max_rows):
    from pypulsar_amd.subfold import plan_blocks
    npart, N, bmax = 7, 50003, 613
    nfold = npart * ((N - bmax) // npart)
    blocks = plan_blocks([nfold], [bmax], max_rows)
    assert blocks[0][0] == 0 and blocks[-1][1] == nfold + bmax
    seen = np.zeros(nfold, dtype=np.int64)
    for k, (a, b, i0, i1) in enumerate(blocks):
        assert 0 < b - a <= max_rows
        if k:
            assert a == blocks[k - 1][1] - bmax             # overlap bmax
        assert a <= i0[0] <= i1[0] and (i1[0] == i0[0] or i1[0] - 1 + bmax < b)
        seen[i0[0]:i1[0]] += 1
    assert np.all(seen == 1)
    if max_rows >= nfold + bmax:
        assert len(blocks) == 1
    # jobs of different delays share the blocks
    bm = np.array([613, 0, 4000])
    nf = npart * ((N - bm) // npart)
    if max_rows > 4000:
        blocks = plan_blocks(nf, bm, max_rows)
        assert blocks[-1][1] == (nf + bm).max()
        for j in range(3):
            seen = np.zeros(nf[j], dtype=np.int64)
            for a, b, i0, i1 in blocks:
                assert i1[j] == i0[j] or (a <= i0[j] and i1[j] - 1 + bm[j] < b)
                seen[i0[j]:i1[j]] += 1
            assert np.all(seen == 1)
    else:
        with pytest.raises(ValueError):
            plan_blocks(nf, bm, max_rows)
    assert plan_blocks([], [], 100) == []


def test_npz_round_trip(tmp_path):
    from pypulsar_amd import subfold as sf
    rng = np.random.default_rng(0)
    npart, nsub, nbins, ndm, C = 4, 8, 16, 17, 64
    fold = sf.SubbandFold(
        dm_fold=55.0, dm=57.79, ddm=2.79, best=9, chi2=5393.25, sigma=88.5, f=19.988, fd=-1e-4,
        T=8.3, dt=256e-6, nsamp=32760, sub=rng.normal(size=(nsub, nbins)),
        subints=rng.normal(size=(npart, nbins)),
        subint_counts=rng.integers(0, 99, (npart, nbins)).astype(np.int32),
        profile=rng.normal(size=nbins), counts=rng.integers(0, 1 << 40, nbins),
        chi2_vs_dm=rng.normal(size=ndm), dms=np.linspace(30, 80, ndm),
        chansum=rng.normal(size=C), chansq=rng.normal(size=C), sub_freqs=np.linspace(1500, 1400, nsub))
    fn = str(tmp_path / "c_subbands.npz")
    sf.write_subfold(fn, fold)
    back = sf.read_subfold(fn)
    with np.load(fn, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(sf._KEYS + sf._SCALARS)
    for k in sf._KEYS:
        a, b = getattr(fold, k), getattr(back, k)
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a, b)
    for k in sf._SCALARS:
        assert getattr(fold, k) == getattr(back, k) and type(getattr(back, k)) in (int, float)
    assert "57.79" in repr(back)


def test_abi_refuses_without_gpu():
    """The limits and the coverage are checked before any HIP call."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from pypulsar_amd import _lib
    h = _lib.lib()

    def job(L=700, i0=0, i1=4900, row=0, bmax=100):
        jb = np.array([[0, 1 << 40, 0, L, i0, i1, row, bmax]], dtype=np.int64)
        return jb, jb.ctypes.data_as(ctypes.c_void_p)

    def fold(dtype=_lib.U8, n=5003, C=64, ld=64, t_first=0, npart=7, nsub=8, nbins=50, jb=None,
             rows=1):
        return h.pdd_subfold(None, dtype, n, C, ld, t_first, jb, None, 1, None, rows, npart, nsub,
                             nbins, None, None, None, None, -1, None)

    def zero(C=64, npart=7, nsub=8, nbins=50):
        return h.pdd_subfold_zero(None, None, None, None, 1, C, npart, nsub, nbins, None)

    def dm(C=64, npart=7, nsub=8, nbins=50, ndm=51):
        return h.pdd_subfold_dm(None, None, None, None, None, None, None, 1, C, npart, nsub, nbins,
                                ndm, None, None, None, None, None, None, None, None)

    for fn in (fold, zero, dm):
        assert fn() == -1 and b"null pointer" in h.pdd_last_error()
        for bad in (dict(nbins=1), dict(nbins=257), dict(npart=0), dict(npart=129),
                    dict(npart=64, nbins=256), dict(nsub=64, nbins=256), dict(nsub=7),
                    dict(nsub=0)):
            assert fn(**bad) == -1 and b"null pointer" not in h.pdd_last_error(), bad
        assert fn(npart=32, nsub=32, nbins=256) == -1 and b"null pointer" in h.pdd_last_error()
    for bad in (dict(ndm=0), dict(ndm=1025)):
        assert dm(**bad) == -1 and b"ndm" in h.pdd_last_error()
    assert dm(ndm=1024) == -1 and b"null pointer" in h.pdd_last_error()
    for bad in (dict(dtype=_lib.U16), dict(n=0), dict(n=1 << 31), dict(ld=63), dict(t_first=-1)):
        assert fold(**bad) == -1 and b"null pointer" not in h.pdd_last_error(), bad
    # per job, on the host copy (a non-null x: the job checks come after the pointers)
    x = np.zeros(16, dtype=np.uint8)
    p = x.ctypes.data_as(ctypes.c_void_p)

    def fold_job(n=5003, t_first=0, **kw):
        jb, jp = job(**kw)
        return h.pdd_subfold(p, _lib.U8, n, 64, 64, t_first, jp, p, 1, p, 1, 7, 8, 50, p, p, p, p,
                             -1, None)

    for bad, word in ((dict(L=0), b"part length"), (dict(row=1), b"table row"),
                      (dict(bmax=-1), b"table row"), (dict(i1=4901), b"outside"),
                      (dict(i0=-1), b"outside"), (dict(i0=10, i1=5), b"outside"),
                      (dict(bmax=104), b"does not cover"), (dict(t_first=1), b"does not cover"),
                      (dict(n=4999), b"does not cover")):
        assert fold_job(**bad) == -1 and word in h.pdd_last_error(), bad
