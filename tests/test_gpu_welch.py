"""mkid_welch_psd on the device (k_welch.hip) against its host twin mkid_welch_psd_host, which
tests/test_welch_host.py holds under the bar against numpy and the long-double truth: bit for bit, on
every shape and input kind of iqnoise_cases.py (the LDS transform up to 4096, the four-step transform
from 8192 with square and non-square splits, one segment, several with an unread tail, two strips),
twice over, for a channel alone, in a block of 3 with a padded row stride, and with group 1, 2 and 0.

Recorded on an MI355X (profiles/iqnoise/new_gputests.txt): every comparison is of bits, and all are
equal; the 12 tests take under 2 s.
"""
import numpy as np
import pytest

import iqnoise_cases as nc
from mkids_sdr_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(64, max_chunk=2 ** 14)
    yield ch
    ch.close()


def dev_psd(ctx, a, b, n, nfft, fs=nc.FS, group=0, want_b=True, fill=-7.0):
    """mkid_welch_psd on [nch][ld] blocks into pre-filled outputs -> (pa, pb)."""
    import torch
    nch, ld = a.shape
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_a, d_b = up(a), up(b)
    nb = max(int(nfft) // 2 + 1, 1) if nfft > 0 else 1
    d_pa = torch.full((nch, nb), fill, dtype=torch.float64, device='cuda')
    d_pb = torch.full((nch, nb), fill, dtype=torch.float64, device='cuda') if want_b else None
    torch.cuda.synchronize()     # torch's stream made them, the context's stream reads them
    try:
        ctx.welch_psd_device(d_a, d_b, n, ld, nch, nfft, fs, group, d_pa, d_pb)
    finally:
        torch.cuda.synchronize()
    return d_pa.cpu().numpy(), None if d_pb is None else d_pb.cpu().numpy()


@pytest.mark.parametrize('nfft,n', nc.SHAPES)
def test_device_equals_host_twin_bit_for_bit(ctx, nfft, n):
    ins, _ = nc.welch_inputs(nfft, n)
    host = nc.host_kinds(nfft, n)
    if nfft == 262144:           # one channel at a time
        for k in nc.KINDS:
            a, b = ins[k]
            for _ in range(2):
                pa, pb = dev_psd(ctx, a[None, :], b[None, :], n, nfft)
                assert nc.same_bits(pa[0], host[k][0]) and nc.same_bits(pb[0], host[k][1]), k
        return
    for kinds in (nc.KINDS[:3], nc.KINDS[3:]):
        A = nc.block([ins[k][0] for k in kinds], n + 1)
        B = nc.block([ins[k][1] for k in kinds], n + 1)
        for group in (0, 0, 1, 2):       # twice over at group 0: a pure function, warm tables
            pa, pb = dev_psd(ctx, A, B, n, nfft, group=group)
            for i, k in enumerate(kinds):
                assert nc.same_bits(pa[i], host[k][0]) and nc.same_bits(pb[i], host[k][1]), (k, group)
        for i, k in enumerate(kinds):    # alone, ld = n
            pa, pb = dev_psd(ctx, ins[k][0][None, :], ins[k][1][None, :], n, nfft)
            assert nc.same_bits(pa[0], host[k][0]) and nc.same_bits(pb[0], host[k][1]), k
    pa, pb = dev_psd(ctx, ins['a_only'][0][None, :], None, n, nfft, want_b=False)
    assert pb is None and nc.same_bits(pa[0], host['a_only'][0])
    assert np.all(dev_psd(ctx, ins['zeros'][0][None, :], None, n, nfft)[0] == 0.0)


def test_argument_errors_launch_nothing(ctx):
    a = nc.block([np.arange(40.0)], 41)
    ok = dict(n=40, nfft=16, fs=nc.FS, group=0)
    bad = [dict(nfft=12), dict(nfft=4), dict(nfft=0), dict(nfft=2 ** 19), dict(n=15), dict(n=42), dict(group=-1),
           dict(fs=0.0), dict(fs=-1.0), dict(fs=float('nan')), dict(fs=float('inf'))]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            dev_psd(ctx, a, a, **{**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    import torch
    d_a = torch.from_numpy(a).cuda()
    out = torch.full((1, 9), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    for args in ((None, None, 40, 41, 1, 16, nc.FS, 0, out, None), (d_a, None, 40, 41, 1, 16, nc.FS, 0, None, None),
                 (d_a, None, 40, 41, 0, 16, nc.FS, 0, out, None), (d_a, d_a, 40, 41, 1, 12, nc.FS, 0, out, out)):
        with pytest.raises(_lib.MkidError) as e:
            ctx.welch_psd_device(*args)
        assert e.value.code == _lib.MKID_E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())          # nothing was launched
    ctx.welch_psd_device(d_a, None, 40, 41, 1, 16, nc.FS, 0, out, None)
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
    rc, pa, _ = nc.host_psd(a, None, 40, 16)
    assert rc == 0 and nc.same_bits(out.cpu().numpy(), pa)
