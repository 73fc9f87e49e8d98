"""The quick-look arithmetic of the reference's dashboard on the energy cube, on the host: the cube
is C x 13 int32 (40 KB for 1024 pixels) and needs no kernel. ArconsDashboard.py image_Worker
(:1282-1505) reads data.bin, total_pix x 10 native uint32 energy or wavelength slices per pixel
(unpack_file, :1331-1337), written by a dataBin.py that the reference does not hold; here the slices
are columns 1 .. 10 of observe.Observation.cube() (include/mkidgpu.h mkid_energy_cube) and
data_bin() writes that file's bytes. Every function restates the lines it cites in numpy float64,
with the sums in the reference's order.
"""
import numpy as np

from . import _lib

H = 4.13567E-15      # [eV s]  ArconsDashboard.py:62
C = 3.0E17           # [nm/s]  ArconsDashboard.py:61
EMIN, EMAX = 0.92, 3.18   # image_Worker.__init__, :1283
NSLICES = 10


def slice_range(bintype='wavelength', Emin=EMIN, Emax=EMAX, h=H, c=C):
    """(binmin, binmax) of setup_thread, :1303-1311: the energies, or by default the wavelengths
    h c / Emax .. h c / Emin."""
    if bintype == 'energy':
        return Emin, Emax
    return h * c / Emax, h * c / Emin


def slice_centres(bintype='wavelength', Emin=EMIN, Emax=EMAX, h=H, c=C):
    """E0 .. E9 of setup_thread, :1312-1322: dE = (binmax - binmin) / 10, E0 = binmin + dE / 2, and
    each further centre the one before plus dE. -> (float64 [10], dE)."""
    binmin, binmax = slice_range(bintype, Emin, Emax, h, c)
    dE = (binmax - binmin) / 10.
    E = [binmin + dE / 2.]
    for _ in range(NSLICES - 1):
        E.append(E[-1] + dE)
    return np.array(E, np.float64), dE


def slice_bins(bintype='wavelength', Emin=EMIN, Emax=EMAX, h=H, c=C):
    """(mode, lo, hi, nb) for observe.Observation(energy_bins=...): the ten slices of setup_thread."""
    lo, hi = slice_range(bintype, Emin, Emax, h, c)
    return (_lib.CUBE_ENERGY if bintype == 'energy' else _lib.CUBE_WAVELENGTH), lo, hi, NSLICES


def slices(cube):
    """The ten slices of a cube int32 [C][13] (columns 1 .. 10: under, over and "no energy" stay
    out, as dataBin's slices hold only binned photons) as uint32 [C][10]."""
    cube = np.asarray(cube)
    if cube.ndim != 2 or cube.shape[1] != NSLICES + 3:
        raise ValueError('quicklook: the cube must be [C][13] (ten bins)')
    return np.ascontiguousarray(cube[:, 1:NSLICES + 1]).view(np.uint32)


def data_bin(cube):
    """The bytes of data.bin: native uint32 [C][10], what unpack_file (:1331-1337) reads with
    struct.unpack(total_pix * '10I')."""
    return slices(cube).astype('=u4').tobytes()


def unpack(data, total_pix):
    """unpack_file, :1335-1336, on the bytes: int64 [total_pix][10]."""
    return np.frombuffer(data, '=u4', count=total_pix * NSLICES).reshape(total_pix, NSLICES).astype(np.int64)


def medians(darray):
    """The median over the pixels of every slice, :1463-1465. float64 [10]."""
    return np.array([np.median(darray[:, k]) for k in range(NSLICES)], np.float64)


def subtract_sky(darray, meds):
    """x - int(med) in every slice, :1338-1353: the median truncated to an integer."""
    return darray - np.array([int(m) for m in meds], np.int64)[None, :]


def photon_counts(darray):
    """pc, :1469-1471: a pixel's total over the ten slices."""
    pc = np.zeros(darray.shape[0], np.int64)
    for k in range(NSLICES):
        pc = pc + darray[:, k]
    return pc


def mean_energy(darray, pc, bintype='wavelength', Emin=EMIN, Emax=EMAX, h=H, c=C):
    """me of calc_mean_energy, :1354-1360: (C0 E0 + C1 E1 + .. + C9 E9) / pc summed left to right,
    and h c over that for wavelength slices. A pixel with pc == 0 gives NaN (the reference divides
    by zero there)."""
    E, _ = slice_centres(bintype, Emin, Emax, h, c)
    acc = darray[:, 0].astype(np.float64) * E[0]
    for k in range(1, NSLICES):
        acc = acc + darray[:, k].astype(np.float64) * E[k]
    me = np.full(darray.shape[0], np.nan, np.float64)
    ok = pc != 0
    me[ok] = acc[ok] / pc[ok].astype(np.float64)
    if bintype != 'energy':
        with np.errstate(divide='ignore'):
            me[ok] = h * c / me[ok]
    return me


def image(cube, sky_subtraction=False, bintype='wavelength', Emin=EMIN, Emax=EMAX, h=H, c=C):
    """image_Worker.run, :1449-1472, on a cube: dict(counts int64 [C][10] (after the sky
    subtraction when asked), medians float64 [10] (before it), pc int64 [C], me float64 [C])."""
    darray = unpack(data_bin(cube), np.asarray(cube).shape[0])
    meds = medians(darray)
    if sky_subtraction:
        darray = subtract_sky(darray, meds)
    pc = photon_counts(darray)
    return dict(counts=darray, medians=meds, pc=pc, me=mean_energy(darray, pc, bintype, Emin, Emax, h, c))


def calculate_snr(totalcounts, meds, npix, sky_subtraction=False):
    """calculate_SNR, :1361-1380: per slice signal = total (less npix median unless the sky was
    subtracted already), floored at 0, noise = npix median (1 where that is 0), SNR = signal /
    sqrt(noise); and the integrated SNR of the sums. -> (float64 [10], float)."""
    total_signal, total_n = 0.0, 0.0
    snr = np.zeros(len(meds), np.float64)
    for i in range(len(meds)):
        noise = npix * float(meds[i])
        signal = float(totalcounts[i]) if sky_subtraction else float(totalcounts[i]) - noise
        if signal < 0:
            signal = 0.0
        if noise == 0:
            noise = 1.0
        total_signal += signal
        total_n += noise
        snr[i] = signal / np.sqrt(noise)
    return snr, total_signal / np.sqrt(total_n)
