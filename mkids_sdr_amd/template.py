"""Pulse template and near-optimal filter on the device.

`make_template` is the reference's MakeTemplate (DataReadout/ReadoutControls/lib/pulses.py:239-427)
for one resonator's pulse set — the RawPulse rows I, Q float32 [P][2000] — returning the
PulseAnalysis fields (pulses.py:44-51). `optimal_filter` fills the step the reference leaves as a
stub (pulses.py:398, PulseAnalysis.coeff Float32Col(100)). `matched_fir_taps` turns the filter
into the firmware's 26-tap matched filter (K7) that `loadFIRcoeffs` / `Channelizer.set_fir` load.
"""
import ctypes

import numpy as np

from . import _lib, codecs

NPTS = 2000
NNOISE = 800


def _dev(a, dtype):
    import torch
    if hasattr(a, 'data_ptr'):
        return a.to(dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32
                                                 else np.float64)).cuda()


def make_template(ch, I, Q):
    """I, Q: float32 [P][2000] (host arrays or device tensors). Returns a dict with template
    [2000], noise [800], noiseidx [800] (np.fft.fftfreq(800, d=2e-6), pulses.py:391) and the
    scalars count, count1, pm, pdev, flag, pstart. I and Q are left as they are. Raises MkidError
    with MKID_E_STATE when no pulse passes the first pass or none passes the second."""
    import torch
    dI, dQ = _dev(I, torch.float32), _dev(Q, torch.float32)
    if dI.dim() != 2 or dI.shape[1] != NPTS or dQ.shape != dI.shape:
        raise ValueError('I, Q must be [P][2000]')
    tpl = torch.empty(NPTS, dtype=torch.float64, device=dI.device)
    noise = torch.empty(NNOISE, dtype=torch.float64, device=dI.device)
    info = _lib.TemplateInfo()
    torch.cuda.synchronize()
    ch._chk(ch._L.mkid_make_template(ch._h, ctypes.c_void_p(dI.data_ptr()), ctypes.c_void_p(dQ.data_ptr()),
                                     int(dI.shape[0]), ctypes.c_void_p(tpl.data_ptr()),
                                     ctypes.c_void_p(noise.data_ptr()), ctypes.byref(info)))
    return dict(template=tpl.cpu().numpy(), noise=noise.cpu().numpy(),
                noiseidx=np.fft.fftfreq(NNOISE, d=0.000002), count=info.count, count1=info.count1,
                pm=info.pm, pdev=info.pdev, flag=info.flag, pstart=info.pstart,
                d_template=tpl, d_noise=noise)


def optimal_filter(ch, template, noise, pre=100, ncoeff=100):
    """Correlation weights of the S/J optimal filter (see include/mkidgpu.h), float64 [ncoeff]."""
    import torch
    t = _dev(template, torch.float64)
    n = _dev(noise, torch.float64)
    out = torch.empty(ncoeff, dtype=torch.float64, device=t.device)
    torch.cuda.synchronize()
    ch._chk(ch._L.mkid_optimal_filter(ch._h, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(n.data_ptr()),
                                      int(pre), int(ncoeff), ctypes.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def iq_from_phase(records, sign=-1.0):
    """Phase records (rad, e.g. one channel of a capture bank) -> unit-circle pulse records
    I = cos(sign phi), Q = sin(sign phi), float32, which `make_template` takes with centre (0, 0).
    sign = -1: phase pulses are negative-going at the trigger and MakeTemplate wants positive peaks."""
    ph = np.float32(sign) * np.asarray(records, np.float32)
    return np.cos(ph), np.sin(ph)


def filters_from_bank(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=None, keep_templates=False):
    """Per-channel optimal filters from a capture bank (Channelizer.capture_bank, records of 2000
    rows): every channel with at least `min_records` ready records goes iq_from_phase ->
    make_template -> optimal_filter (one pair of launches per channel) and fills its row of coeff
    [C][ncoeff] float32, ready for Channelizer.set_pulse_filter (the weights start 10 rows before
    the template peak). A channel with fewer records, or on which make_template raises (no
    surviving pulse), takes its row from `fallback` ([C][ncoeff] or [ncoeff]; default zeros).
    Returns dict(coeff, count [C] float64, flag [C] int32, pstart [C] int32, ready [C] int32,
    used [C] bool); flag and pstart are -1 where the fallback was taken. keep_templates adds
    templates {channel: (template [2000], noise [800])}."""
    records, _, info = bank
    C = records.shape[0]
    if records.shape[2] != NPTS:
        raise ValueError('filters_from_bank needs records of %d rows (set_capture(length=%d))' % (NPTS, NPTS))
    ready = info.cpu().numpy()[:, 0].astype(np.int32)
    coeff = np.zeros((C, ncoeff), np.float32)
    if fallback is not None:
        coeff[:] = np.asarray(fallback, np.float32)
    count = np.zeros(C, np.float64)
    flag = np.full(C, -1, np.int32)
    pstart = np.full(C, -1, np.int32)
    used = np.zeros(C, bool)
    templates = {}
    for c in np.flatnonzero(ready >= max(int(min_records), 1)):
        I, Q = iq_from_phase(records[c, :ready[c]].cpu().numpy())
        try:
            r = make_template(ch, I, Q)
        except _lib.MkidError as e:
            if e.code != _lib.MKID_E_STATE:
                raise
            continue
        coeff[c] = optimal_filter(ch, r['d_template'], r['d_noise'], pre=pre, ncoeff=ncoeff)
        count[c], flag[c], pstart[c], used[c] = r['count'], r['flag'], r['pstart'], True
        if keep_templates:
            templates[int(c)] = (r['template'], r['noise'])
    out = dict(coeff=coeff, count=count, flag=flag, pstart=pstart, ready=ready, used=used)
    if keep_templates:
        out['templates'] = templates
    return out


RESULT_DTYPE = np.dtype([('count', np.float64), ('count1', np.float64), ('pm', np.float64), ('pdev', np.float64),
                         ('flag', np.int32), ('pstart', np.int32), ('status', np.int32), ('ready', np.int32)])


def result_table(d_result):
    """The device result table of `bank_filters` ([Cb][48] uint8) as a numpy record array with the
    fields of mkid_bank_result."""
    return d_result.cpu().numpy().view(RESULT_DTYPE).reshape(-1)


def bank_filters(ch, I, Q, ready, *, pre=100, ncoeff=100, min_records=20, fallback=None, keep_templates=False,
                 group=0, sign=-1.0, ready_stride=None, sync=True):
    """mkid_bank_filters (include/mkidgpu.h) on device tensors: I, Q float32 [Cb][R][2000], or Q =
    None and I holding phase records (rad); ready int32 [Cb] or a capture info [Cb][2]
    (ready_stride defaults to its row length). Every channel with enough records gets its row of
    coeff [Cb][ncoeff] float32; the others keep `fallback` ([Cb][ncoeff] or [ncoeff]; default zeros).
    Returns dict(coeff, result) of device tensors (result: see `result_table`), plus templates
    [Cb][2000] and noise [Cb][800] float64 with keep_templates (rows of unused channels are NaN).
    Nothing passes through the host. sync=False leaves the call running on the context stream."""
    import torch
    if I.dim() != 3 or I.shape[2] != NPTS or I.dtype != torch.float32 or not I.is_contiguous():
        raise ValueError('records must be contiguous float32 [Cb][R][2000]')
    if Q is not None and (Q.shape != I.shape or Q.dtype != torch.float32 or not Q.is_contiguous()):
        raise ValueError('Q must match I')
    Cb, R = int(I.shape[0]), int(I.shape[1])
    if ready.dtype != torch.int32 or not ready.is_contiguous() or ready.shape[0] != Cb:
        raise ValueError('ready must be contiguous int32 [Cb] or [Cb][k]')
    if ready_stride is None:
        ready_stride = 1 if ready.dim() == 1 else int(ready.shape[1])
    dev = I.device
    coeff = torch.zeros((Cb, int(ncoeff)), dtype=torch.float32, device=dev)
    if fallback is not None:
        fb = fallback if hasattr(fallback, 'data_ptr') else torch.from_numpy(np.asarray(fallback, np.float32))
        coeff[:] = fb.to(device=dev, dtype=torch.float32)
    tpl = torch.full((Cb, NPTS), float('nan'), dtype=torch.float64, device=dev) if keep_templates else None
    noise = torch.full((Cb, NNOISE), float('nan'), dtype=torch.float64, device=dev) if keep_templates else None
    result = torch.zeros((Cb, ctypes.sizeof(_lib.BankResult)), dtype=torch.uint8, device=dev)
    cfg = _lib.BankCfg(Cb, R, NPTS, int(min_records), int(pre), int(ncoeff), int(ready_stride), int(group),
                       float(sign))
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    torch.cuda.synchronize(dev)   # the tensors were made on torch's stream, the kernels run on the context's
    ch._chk(ch._L.mkid_bank_filters(ch._h, p(I), p(Q), p(ready), ctypes.byref(cfg), p(tpl), p(noise), p(coeff),
                                    p(result)))
    if sync:
        torch.cuda.synchronize(dev)
    out = dict(coeff=coeff, result=result)
    if keep_templates:
        out.update(templates=tpl, noise=noise)
    return out


def filters_from_bank_device(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=None, keep_templates=False,
                             load=False):
    """`filters_from_bank` in one device call: the bank's phase records go through
    mkid_bank_filters in phase mode where they lie (ready read from the bank's info, no per-channel
    host step), then the small outputs are copied once. Same arguments, same dict, plus status [C]
    int32 (mkid_bank_result.status; used = status == 0). load=True also makes the table the
    context's pulse filter where it lies (Channelizer.set_pulse_filter_device with pre = 10, the
    rows the weights start before the template peak): it does not leave the device for that."""
    records, _, info = bank
    if records.shape[2] != NPTS:
        raise ValueError('filters_from_bank_device needs records of %d rows (set_capture(length=%d))' % (NPTS, NPTS))
    r = bank_filters(ch, records, None, info, pre=pre, ncoeff=ncoeff, min_records=min_records, fallback=fallback,
                     keep_templates=keep_templates, sign=-1.0)
    if load:
        ch.set_pulse_filter_device(r['coeff'], pre=10)
    t = result_table(r['result'])
    used = t['status'] == 0
    out = dict(coeff=r['coeff'].cpu().numpy(), count=t['count'].copy(), flag=t['flag'].copy(),
               pstart=t['pstart'].copy(), ready=t['ready'].copy(), used=used, status=t['status'].copy())
    if keep_templates:
        tp, nz = r['templates'].cpu().numpy(), r['noise'].cpu().numpy()
        out['templates'] = {int(c): (tp[c], nz[c]) for c in np.flatnonzero(used)}
    return out


def matched_fir_taps(coeff, ntaps=26, sign=-1.0):
    """Firmware FIR taps from correlation weights: the ntaps-long window of largest energy,
    reversed into convolution order (f_j = sum_i a_i raw_{j-i}), scaled to max |a| = 2047/2048
    and multiplied by `sign` (phase pulses are negative-going at the trigger, ROACH_Pulses.py:270).
    Returns (float taps for loadFIRcoeffs, int12 taps for Channelizer.set_fir)."""
    c = np.asarray(coeff, np.float64)
    e = np.convolve(c * c, np.ones(ntaps), mode='valid')
    k = int(np.argmax(e))
    a = sign * c[k:k + ntaps][::-1]
    a = a / np.max(np.abs(a)) * (2047.0 / 2048.0)
    return a, codecs.fir_quantise(a)
