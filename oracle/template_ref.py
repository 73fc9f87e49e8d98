"""Restatement of the reference's MakeTemplate (DataReadout/ReadoutControls/lib/pulses.py:239-427)
— TEST INFRASTRUCTURE (oracle for k_template.hip).

Input: one resonator's pulses as the reference's RawPulse table holds them (pulses.py:30-43):
I, Q float32 [P][2000]. The PyTables file I/O is replaced by arrays; the arithmetic follows the
reference line by line in numpy with the reference's dtypes (float32 pulses, float64 fit and
template), including its quirk that `I = dat['I'][j]; I += ...` edits the table in place, so the
first 1000 pulses are re-referenced twice (once per pass).

Parity: the reference is Python 2 + PyTables and cannot run here; this restatement is pinned by
the reference's own FakeTemplateData generator (pulses.py:429-481, restated and extended in
tests/template_pulses.py), not by reference outputs (DESIGN.md §4.6 says what pins the device
against this file).

The optimal filter is a stub in the reference (pulses.py:398 "calculate optimal filter
parameters", PulseAnalysis.coeff = Float32Col(100), pulses.py:59): `optimal_filter` below is this
repository's definition, the frequency-domain matched filter S*/J.
"""
import numpy as np

NPTS = 2000
NNOISE = 800


# per-pulse decision codes (dec1: first pass, dec2: second pass), in the order the reference tests
ACCEPT, BAD_BASELINE, PEAK_LOW, PEAK_HIGH, PLOC1_OUT, PEAK_OUTLIER, PLOC2_OUT = range(7)
NOLOC = -9999   # ploc1 / ploc2 of a pulse rejected before its peak was located


def make_template(I, Q, xc=0.0, yc=0.0, phase_hook=None):
    """Besides the reference's outputs: dec1 [min(P, 1000)] and dec2 [P] int8, the decision taken
    on every pulse in each pass (codes above), and nwrap [P], the number of samples of the pulse
    at which np.unwrap applied a non-zero correction in the second pass, and ploc1 / ploc2, the
    peak location each pass found (NOLOC where it did not get that far). `phase_hook`, if given,
    maps the float32 arctan2 output of one pulse to the array used in its place (the tests perturb
    it by a few ulp to show that no decision hangs on the last bits of atan2). Raises ValueError
    when no pulse passes a pass (the reference divides by zero and then fails on an empty
    np.where)."""
    dat_I = np.array(I, np.float32, copy=True)   # the table read into memory (pulses.py:263)
    dat_Q = np.array(Q, np.float32, copy=True)
    N = len(dat_I)
    tP = np.zeros(NPTS, dtype='float64')
    tPf = np.zeros(NPTS, dtype='float64')
    noise = np.zeros(NNOISE, dtype='float64')
    count = 0.0
    peaklist = []
    idx = np.arange(NPTS) * 2.0                                          # :269
    fitidx = np.concatenate((idx[:900], idx[1800:]))                     # :270
    I1m = np.median(dat_I[:100, :900])                                   # :277
    Q1m = np.median(dat_Q[:100, :900])
    if N > 1000:                                                         # :281
        N = 1000

    nwrap = np.zeros(len(dat_I), np.int64)
    dec1 = np.zeros(N, np.int8)
    dec2 = np.zeros(len(dat_I), np.int8)
    ploc1 = np.full(N, NOLOC)
    ploc2 = np.full(len(dat_I), NOLOC)

    def prep(j):
        Ij = dat_I[j]                 # views: the += below edits the table (pulses.py:287-292)
        Qj = dat_Q[j]
        Ij += (I1m - np.median(Ij[1:900]))
        Qj += (Q1m - np.median(Qj[1:900]))
        P1 = np.arctan2(Qj - yc, Ij - xc)                                # :295
        if phase_hook is not None:
            P1 = phase_hook(P1)
        U = np.unwrap(P1)
        nwrap[j] = np.count_nonzero(U != P1)
        P2 = np.rad2deg(U)                                               # :299
        fit = np.poly1d(np.polyfit(fitidx, np.concatenate((P2[:900], P2[1800:])), 1))  # :302
        P3 = P2 - fit(idx)
        stdev = np.std(P3[:100])                                         # :306
        bad = np.abs(np.mean(P3[:100]) - np.mean(P3[1900:])) > stdev * 2.0
        return P3, bad

    for j in range(N):                                                   # first pass :285
        P3, bad = prep(j)
        if bad:
            dec1[j] = BAD_BASELINE
            continue
        peak = np.max(P3[980:1050])                                      # :313
        peaklist.append(peak)
        if peak < 15.0 or peak > 120.0:
            dec1[j] = PEAK_LOW if peak < 15.0 else PEAK_HIGH
            continue
        ploc = int(np.where(P3 == peak)[0][0])                           # :319
        ploc1[j] = ploc
        if ploc < 980 or ploc > 1020:
            dec1[j] = PLOC1_OUT
            continue
        P4 = np.roll(P3, 1000 - ploc)                                    # :324
        tP += P4 / np.max(P4)
        count += 1
    count1 = count
    if count == 0:
        raise ValueError('make_template: no pulse passed the first pass')
    tP /= count                                                          # :330

    peaklist = np.asarray(peaklist)                                      # :334
    pm = np.median(peaklist[np.where(peaklist > 15)])
    pdev = np.std(peaklist[np.where(peaklist > 15)])

    N = len(dat_I)                                                       # :339
    count = 0.0
    for j in range(N):                                                   # second pass
        P3, bad = prep(j)
        if bad:
            dec2[j] = BAD_BASELINE
            continue
        conv = np.convolve(tP[900:1500], P3)                             # :366
        ploc = int(np.where(conv == np.max(conv))[0][0] - 1160.0)
        ploc2[j] = ploc
        peak = np.max(P3[1000 + ploc])
        if peak < pm - 4.0 * pdev or peak > pm + 4.0 * pdev:             # :372
            dec2[j] = PEAK_OUTLIER
            continue
        if ploc < -30 or ploc > 30:                                      # :376
            dec2[j] = PLOC2_OUT
            continue
        P4 = np.roll(P3, -ploc)                                          # :380
        tPf += P4 / np.max(P4)
        count += 1
        noise += np.abs(np.fft.fft(np.deg2rad(P4[50:850]))) ** 2         # :387
    if count == 0:
        raise ValueError('make_template: no pulse passed the second pass')
    tPf /= count
    noise /= count
    noiseidx = np.fft.fftfreq(len(noise), d=0.000002)                    # :391
    flag = 1 if (count < 500 or pm < 10 or pm > 150) else 0              # :409
    pstart = int(np.where(tPf == np.max(tPf))[0][0])
    return dict(template=tPf, noise=noise, noiseidx=noiseidx, count1=count1, count=count,
                pm=pm, pdev=pdev, flag=flag, pstart=pstart, template1=tP,
                dec1=dec1, dec2=dec2, nwrap=nwrap, ploc1=ploc1, ploc2=ploc2)


def optimal_filter(template, noise, ncoeff=100, pre=100):
    """S*/J matched filter from the template and the noise PSD (this repository's definition; the
    reference's step is a stub): s = template[pstart - pre : pstart - pre + 800] (deg -> rad),
    H = S / J with H[0] = 0 (baseline-insensitive), g = real(ifft(H)) read as correlation weights
    (y_j = sum_m g[m] x_{j+m} = ifft(conj(S) X / J)_j: white noise gives g = s, the plain matched
    filter); normalised so that sum_m g[m] s[m] = 1 (unit gain for a template-shaped pulse); the
    ncoeff weights starting pre-10 samples before the peak. Where the window leaves the record
    the samples outside [0, 2000) are zero, and so are the weights g[m] at m >= 800 (a window
    inside the record takes the slice itself, as before)."""
    t = np.asarray(template, np.float64)
    J = np.asarray(noise, np.float64)
    pstart = int(np.argmax(t))
    p0 = pstart - pre
    if p0 >= 0 and p0 + NNOISE <= NPTS:
        s = np.deg2rad(t[p0:p0 + NNOISE])
    else:
        s = np.zeros(NNOISE)
        lo, hi = max(p0, 0), min(p0 + NNOISE, NPTS)
        s[lo - p0:hi - p0] = np.deg2rad(t[lo:hi])
    S = np.fft.fft(s)
    H = S / J            # applied to data as conj(H) X: the S*/J filter
    H[0] = 0.0
    g = np.real(np.fft.ifft(H))
    g /= np.dot(g, s)
    k0 = pre - 10
    out = g[k0:k0 + ncoeff].copy()
    if len(out) < ncoeff:
        out = np.concatenate((out, np.zeros(ncoeff - len(out))))
    return out
