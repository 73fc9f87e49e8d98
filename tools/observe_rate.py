#!/usr/bin/env python3
"""Time the stage after the heights (k_observe.hip: count image, pulse-height spectra, list join)
against mkid_pulse_heights on the same list, in one process, at config 5's shape: phase
[2^18][2048] (one 2^30-sample step at N = 4096), ncoeff = 100, pre = 20, 690 000 packets with
ascending stamps spread over the channels, nbins = 256, a three-second image. The list is timed in
two orders: `dev`, the device's own (channel-major, time-ascending in a channel: what mkid_process
hands to the stage) and `time`, the same packets by ascending stamp (tools/heights_fit_rate.py's list;
the worst case for the count kernel's runs and the spectra kernel's LDS rows).

  heights        mkid_pulse_heights alone: the yardstick on the same list
  count_*        mkid_count_photons
  spectra_lds_*  mkid_height_spectra with the LDS table   (a context made under MKID_OBS_LDS=1)
  spectra_plain_*  the same kernel, one global atomic per packet (MKID_OBS_LDS=0)
  spectra_defer  the shipped form with a deferred list (the packets of the last ncoeff - pre rows wait)
  concat         mkid_concat_packets of 5000 + 690 000 packets
  list_*         mkid_list_photons (k_photons.hip) into [3][C][--row-slots] rows: the call that replaces
                 mkid_count_photons in a step that keeps the photon rows
  fill_*         mkid_fill_photon_heights of the list in that order into the device-order rows
  host_route     what this replaces: device-to-host copy of list and heights, then the numpy restatement
                 (tests/observe_cases.py), wall clock
  pack / drain   with --ring (k_pack.hip): list_ring_* and fill_ring_* (the ring forms over the same window,
                 beside list_* and fill_*), pack, clear and pack_clear of second 1 of the device-order rows
                 (mkid_pack_second, mkid_clear_second), and, wall clock, a whole drain of that second
                 (observe.Observation's: pack, clear, one synchronisation, the photons copied) against the
                 route without it (Observation.rows(sec) plus the padded stamp, height and dt tables of the
                 second), with the bytes each moves to the host
  *_parent       with --parent-lib PATH: list_* and fill_* through a library built from the parent commit,
                 alternating with this tree's in the same rounds

Every device path is one HIP-event interval on a stream shared with torch; the paths alternate inside
each of --reps rounds after two warm-up rounds, and the median, minimum and maximum over the rounds
are reported. On the way all paths must give the same integers as the numpy restatement. Prints one
JSON line and, with --out, writes it.

    python tools/observe_rate.py [--reps 20] [--packets 690000] [--out profiles/observe/observe_rate_c5.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from heights_fit_rate import event_ms, stats  # noqa: E402


def context(C, stream, lds=None):
    from mkids_sdr_amd.channelizer import Channelizer
    old = os.environ.pop('MKID_OBS_LDS', None)
    if lds is not None:
        os.environ['MKID_OBS_LDS'] = '1' if lds else '0'
    try:
        ch = Channelizer(C, max_chunk=1 << 20)
    finally:
        os.environ.pop('MKID_OBS_LDS', None)
        if old is not None:
            os.environ['MKID_OBS_LDS'] = old
    ch.set_stream(stream.cuda_stream)
    return ch


def ring_section(args, chan, s, rows, row_h, want, n_seconds, K, sec=1):
    """Second `sec` of the device-order rows (filled, as the checks left them): pack, clear and both as
    HIP-event intervals, then a whole drain against the route without it as wall clock, the paths
    alternating inside each round after two warm-up rounds. The drain and the other route are
    observe.Observation's own code, run on an Observation that is handed these tables."""
    import torch
    import ring_cases as rc_
    from mkids_sdr_amd import observe
    C = chan.C
    row_dt = torch.full((n_seconds, C, K), float('nan'), device='cuda')
    obs = object.__new__(observe.Observation)      # no step() is run: only the readouts' fields
    obs.chan, obs.K, obs.R, obs.n_seconds, obs.d_pack = chan, K, None, n_seconds, None
    obs.d_image, obs.d_words, obs.d_stamps = rows['image'], rows['words'], rows['stamps']
    obs.d_row_height, obs.d_row_dt = row_h, row_dt
    obs._pack_buffers()
    torch.cuda.synchronize()
    b = obs.d_pack
    keep_image, keep_h = rows['image'][sec].clone(), row_h[sec].clone()

    def restore():
        rows['image'][sec].copy_(keep_image)
        row_h[sec].copy_(keep_h)

    def pack():
        chan.pack_second(sec, n_seconds, K, obs.d_image, obs.d_words, obs.d_stamps, row_h, row_dt, b['cap'], b['counts'],
                         b['offsets'], b['word'], b['stamp'], b['height'], b['dt'], b['total'])

    def clear():
        chan.clear_second(sec, n_seconds, K, obs.d_image, row_h, row_dt)

    def parent_route():                            # Observation.rows(sec) and the three other padded tables of the second
        r = obs.rows(sec)
        return r, obs.d_stamps[sec].cpu().numpy(), row_h[sec].cpu().numpy(), row_dt[sec].cpu().numpy()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    ev_paths = [('pack', pack), ('clear', clear), ('pack_clear', lambda: (pack(), clear()))]
    times = {k: [] for k in ('pack', 'clear', 'pack_clear', 'drain_wall', 'parent_route_wall')}
    for rep in range(args.reps + 2):
        for name, fn in ev_paths:
            restore()
            t = event_ms(s, fn)
            if rep >= 2:
                times[name].append(t)
        restore()
        t_d, second = wall(lambda: obs._packed(sec, n_seconds, True))
        restore()
        t_p, padded = wall(parent_route)
        if rep >= 2:
            times['drain_wall'].append(t_d)
            times['parent_route_wall'].append(t_p)
    restore()
    torch.cuda.synchronize()
    ref = rc_.pack_ref(want, sec)                  # the numpy restatement of the packed second
    m = int(ref.total[0])
    same = (np.array_equal(second.counts, ref.counts) and np.array_equal(second.offsets, ref.offsets) and
            np.array_equal(second.word, ref.words[:m]) and np.array_equal(second.stamp, ref.stamps[:m]) and
            np.array_equal(second.height.view(np.uint32), ref.height[:m].view(np.uint32)))
    same_rows = all(np.array_equal(a, c) for a, c in zip(second.rows(), padded[0]))
    out = {}
    for name, t in times.items():
        out.update(stats(name, t))
    out.update(drain_second=sec, drain_photons=m, drain_bytes=4 * C + 8 * (C + 1) + 24 * m,
               parent_route_bytes=4 * C + 24 * C * K,
               drain_over_parent_route=round(float(np.median(times['drain_wall']) / np.median(times['parent_route_wall'])), 3),
               checks=dict(packed_equal_numpy=bool(same), packed_rows_equal_rows=bool(same_rows)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--packets', type=int, default=690000)
    ap.add_argument('--channels', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--ncoeff', type=int, default=100)
    ap.add_argument('--pre', type=int, default=20)
    ap.add_argument('--nbins', type=int, default=256)
    ap.add_argument('--row-slots', type=int, default=2499)      # PacketMaster's MAX_EVENTS_PER_SEC - 1
    ap.add_argument('--ring', action='store_true', help='also time the ring forms, pack, clear and a whole drain')
    ap.add_argument('--parent-lib', default=None, help='a libmkidgpu.so of the parent commit: list_* / fill_* A/B')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import observe_cases as oc
    C, J, nco, pre, n, nbins = args.channels, args.rows, args.ncoeff, args.pre, args.packets, args.nbins
    n_seconds, n_a = 3, 5000
    rng = np.random.default_rng(0)
    coeff = rng.normal(size=(C, nco)).astype(np.float32)
    s = torch.cuda.Stream()
    ctx = {'default': context(C, s), 'lds': context(C, s, True), 'plain': context(C, s, False)}
    ctx['default'].set_pulse_filter(coeff, pre)
    N, fs = ctx['default'].N, int(ctx['default'].cfg.sample_rate)
    d_ph = torch.randn(J, C, device='cuda')
    chs = rng.integers(0, C, n).astype(np.uint64)
    ts = np.sort(rng.integers(pre, J, n)).astype(np.int64)         # the last nco - pre rows: no height yet
    ev = {'time': (chs << np.uint64(52)) | ts.astype(np.uint64)}
    ev['dev'] = oc.device_order(ev['time'], 0)
    j_defer = J + pre - nco + 1
    lo = np.full(C, -32.0, np.float32) + rng.uniform(0, 1, C).astype(np.float32)
    inv = np.full(C, np.float32(1) / np.float32(0.25), np.float32)
    d_lo, d_inv = torch.from_numpy(lo).cuda(), torch.from_numpy(inv).cuda()
    d_ev = {o: torch.from_numpy(e.view(np.int64)).cuda() for o, e in ev.items()}
    d_h = {o: torch.empty(n, dtype=torch.float32, device='cuda') for o in ev}
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')
    names = ['count_dev', 'count_time', 'spectra_lds_dev', 'spectra_lds_time', 'spectra_plain_dev', 'spectra_plain_time',
             'spectra_defer']
    image = {k: z((n_seconds, C), torch.int32) for k in names if k.startswith('count')}
    outside = {k: z(2, torch.int64) for k in image}
    spectra = {k: z((C, nbins + 3), torch.int32) for k in names if k.startswith('spectra')}
    d_def, d_ndef = z(n, torch.int64), z(2, torch.int64)
    d_a, d_na, d_nb = d_ev['time'][:n_a].clone(), torch.tensor([n_a], device='cuda'), torch.tensor([n], device='cuda')
    d_join, d_njoin = z(n + n_a, torch.int64), z(2, torch.int64)
    torch.cuda.synchronize()
    for o in ev:                               # the heights both orders are binned from
        ctx['default'].pulse_heights_device(d_ph, J, 0, d_ev[o], n, d_h[o])
    torch.cuda.synchronize()

    def count(o):
        k = 'count_' + o
        return lambda: ctx['default'].count_photons_device(d_ev[o], n, 0, n_seconds, image[k], outside[k])

    def spec(form, o):
        k = 'spectra_%s_%s' % (form, o)
        return lambda: ctx[form].height_spectra_device(d_ev[o], d_h[o], n, 0, 0, d_lo, d_inv, nbins, spectra[k])

    def spec_defer():
        ctx['default'].height_spectra_device(d_ev['dev'], d_h['dev'], n, 0, j_defer, d_lo, d_inv, nbins,
                                             spectra['spectra_defer'], d_def, n, d_ndef)

    paths = [('heights', lambda: ctx['default'].pulse_heights_device(d_ph, J, 0, d_ev['dev'], n, d_h['dev']))]
    paths += [('count_' + o, count(o)) for o in ('dev', 'time')]
    paths += [('spectra_%s_%s' % (f, o), spec(f, o)) for o in ('dev', 'time') for f in ('lds', 'plain')]
    paths += [('spectra_defer', spec_defer),
              ('concat', lambda: ctx['default'].concat_packets(d_a, d_na, n_a, d_ev['dev'], d_nb, n, d_join, n + n_a, d_njoin))]

    # the photon rows: mkid_list_photons in both orders, each into tables of its own whose image is
    # zeroed before every call (outside the timed interval), so that every round fills the same slots;
    # mkid_fill_photon_heights of both list orders into the rows the device-order list made
    # (stamp-ascending rows are its precondition; the order of its own list is free)
    import photon_cases as pc
    K = args.row_slots
    rows = {o: {k: z(shape, dt) for k, shape, dt in (('image', (n_seconds, C), torch.int32), ('outside', 2, torch.int64),
                                                     ('words', (n_seconds, C, K), torch.int64),
                                                     ('stamps', (n_seconds, C, K), torch.int64),
                                                     ('dropped', 1, torch.int64))} for o in ev}
    row_h = {o: torch.full((n_seconds, C, K), float('nan'), device='cuda') for o in ev}
    d_fill = {o: z(2, torch.int64) for o in ev}

    def rows_list(o):
        r = rows[o]
        return lambda: ctx['default'].list_photons_device(d_ev[o], n, 0, n_seconds, K, pc.WIDE, r['image'], r['outside'],
                                                          r['words'], r['stamps'], r['dropped'])

    def rows_fill(o):
        r = rows['dev']
        return lambda: ctx['default'].fill_photon_heights_device(d_ev[o], d_h[o], None, n, 0, j_defer, n_seconds, K,
                                                                 r['image'], r['stamps'], row_h[o], None, d_fill[o])

    paths += [('list_' + o, rows_list(o)) for o in ev] + [('fill_' + o, rows_fill(o)) for o in ev]
    prep = {'list_' + o: rows[o]['image'].zero_ for o in ev}
    if args.parent_lib:                        # the same calls through the parent's library, same tables
        from mkids_sdr_amd.channelizer import Channelizer
        ctx['parent'] = Channelizer(C, max_chunk=1 << 20, lib_path=args.parent_lib)
        ctx['parent'].set_stream(s.cuda_stream)

        def parent_list(o):
            r = rows[o]
            return lambda: ctx['parent'].list_photons_device(d_ev[o], n, 0, n_seconds, K, pc.WIDE, r['image'], r['outside'],
                                                             r['words'], r['stamps'], r['dropped'])

        def parent_fill(o):
            r = rows['dev']
            return lambda: ctx['parent'].fill_photon_heights_device(d_ev[o], d_h[o], None, n, 0, j_defer, n_seconds, K,
                                                                    r['image'], r['stamps'], row_h[o], None, d_fill[o])

        paths += [('list_%s_parent' % o, parent_list(o)) for o in ev] + [('fill_%s_parent' % o, parent_fill(o)) for o in ev]
        prep.update({'list_%s_parent' % o: rows[o]['image'].zero_ for o in ev})
    if args.ring:                              # the ring forms over the same window: the same work
        out4 = z(4, torch.int64)

        def ring_list(o):
            r = rows[o]
            return lambda: ctx['default'].list_photons_ring_device(d_ev[o], n, 0, 0, n_seconds, n_seconds, K, pc.WIDE,
                                                                   r['image'], out4, r['words'], r['stamps'], r['dropped'])

        def ring_fill(o):
            r = rows['dev']
            return lambda: ctx['default'].fill_photon_heights_ring_device(d_ev[o], d_h[o], None, n, 0, j_defer, 0, n_seconds,
                                                                          n_seconds, K, r['image'], r['stamps'], row_h[o],
                                                                          None, d_fill[o])

        paths += [('list_ring_' + o, ring_list(o)) for o in ev] + [('fill_ring_' + o, ring_fill(o)) for o in ev]
        prep.update({'list_ring_' + o: rows[o]['image'].zero_ for o in ev})
    times = {name: [] for name, _ in paths}
    for rep in range(args.reps + 2):           # two warm-up rounds: code objects, clocks, caches
        for name, fn in paths:
            if name in prep:
                prep[name]()
            t = event_ms(s, fn)
            if rep >= 2:
                times[name].append(t)

    # the route this replaces, and the integers every path must give
    host_t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_ev, h_h = d_ev['dev'].cpu().numpy().view(np.uint64), d_h['dev'].cpu().numpy()
        t1 = time.perf_counter()
        ref_image, ref_out = oc.count_ref(h_ev, 0, N, fs, C, n_seconds)
        ref_sp, _, _ = oc.spectra_ref(h_ev, h_h, 0, 0, C, lo, inv, nbins)
        host_t.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    ref_dsp, ref_def, ref_ndef = oc.spectra_ref(h_ev, h_h, 0, j_defer, C, lo, inv, nbins, defer=True, cap_def=n)
    for t in list(image.values()) + list(outside.values()) + list(spectra.values()) + [d_ndef] + list(d_fill.values()) + \
            [r[k] for r in rows.values() for k in ('image', 'outside', 'dropped')]:
        t.zero_()
    for t in row_h.values():
        t.fill_(float('nan'))
    torch.cuda.synchronize()
    once = [(name, fn) for name, fn in paths[1:] if '_parent' not in name and '_ring_' not in name]
    for name, fn in once:
        if not name.startswith('fill_'):
            fn()
    for name, fn in once:                      # the fills after both lists
        if name.startswith('fill_'):
            fn()
    torch.cuda.synchronize()
    # the rows against the host twins (tests/photon_cases.py): bit for bit in the device's order; by
    # stamp the counters, and every row as a set (K holds every cell here, or `dropped` would differ)
    _, want = pc.list_host(h_ev, 0, N, fs, C, n_seconds, K, pc.WIDE)
    assert pc.fill_host(h_ev, h_h, None, 0, j_defer, N, fs, C, want) == 0
    live = np.arange(K) < np.minimum(want.image, K)[..., None]
    got = {o: {k: t.cpu().numpy() for k, t in rows[o].items()} for o in ev}
    counters = all(np.array_equal(got[o][k], getattr(want, k)) for o in ev for k in ('image', 'outside', 'dropped'))
    by_row = lambda a: np.sort(np.where(live, a, np.iinfo(np.int64).max), axis=-1)
    rows_check = dict(
        rows_counters_equal_host=bool(counters),
        rows_dev_equal_host=bool(np.array_equal(got['dev']['words'].view(np.uint64)[live], want.words[live]) and
                                 np.array_equal(got['dev']['stamps'][live], want.stamps[live])),
        rows_time_same_sets=bool(np.array_equal(by_row(got['time']['stamps']), by_row(want.stamps)) and
                                 np.array_equal(by_row(got['time']['words']), by_row(want.words.view(np.int64)))),
        fill_equal_host=bool(all(np.array_equal(row_h[o].cpu().numpy().view(np.uint32), want.height.view(np.uint32)) and
                                 np.array_equal(d_fill[o].cpu().numpy(), want.fill) for o in ev)),
        rows_dropped=int(want.dropped[0]), rows_filled=int(want.fill[0]), rows_not_found=int(want.fill[1]))
    nd = d_ndef.cpu().numpy()
    check = dict(
        images_equal_numpy=bool(all(np.array_equal(t.cpu().numpy(), ref_image) for t in image.values())),
        outside_equal_numpy=bool(all(np.array_equal(t.cpu().numpy(), ref_out) for t in outside.values())),
        spectra_equal_numpy=bool(all(np.array_equal(spectra[k].cpu().numpy(), ref_sp) for k in names[2:6])),
        deferred_equal_numpy=bool(np.array_equal(spectra['spectra_defer'].cpu().numpy(), ref_dsp) and
                                  np.array_equal(nd, ref_ndef) and
                                  np.array_equal(d_def[:int(nd[1])].cpu().numpy().view(np.uint64), ref_def)),
        concat=bool(np.array_equal(d_join.cpu().numpy().view(np.uint64), np.concatenate([ev['time'][:n_a], ev['dev']])) and
                    d_njoin.cpu().tolist() == [n + n_a, n + n_a]),
        packets_in_image=int(ref_image.sum()), packets_late=int(ref_out[1]), no_height=int(ref_sp[:, nbins + 2].sum()),
        deferred=int(ref_ndef[0]), channels_with_packets=int((ref_sp.sum(axis=1) > 0).sum()))
    check.update(rows_check)
    ring_out = ring_section(args, ctx['default'], s, rows['dev'], row_h['dev'], want, n_seconds, K) if args.ring else {}
    check.update(ring_out.pop('checks', {}))
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = dict(tool='observe_rate', channels=C, rows=J, ncoeff=nco, pre=pre, packets=n, nbins=nbins, n_seconds=n_seconds,
               reps=args.reps)
    for name, t in times.items():
        out.update(stats(name, t))
        out[name + '_mpackets_per_s'] = round(n / med[name] / 1e3, 1)
    for o in ('dev', 'time'):
        l, p = times['spectra_lds_' + o], times['spectra_plain_' + o]
        out['lds_over_plain_' + o] = round(med['spectra_lds_' + o] / med['spectra_plain_' + o], 3)
        out['lds_range_clear_of_plain_' + o] = bool(max(l) < min(p))
    out['row_slots'] = K
    for o in ev:                               # the list call replaces the count call of a step
        out['list_over_count_' + o] = round(med['list_' + o] / med['count_' + o], 3)
    out['stage_over_heights'] =round((med['count_dev'] + med['concat'] + med['spectra_defer']) / med['heights'], 3)
    out['host_route_copy_ms'] = round(float(np.median([a for a, _ in host_t])), 2)
    out['host_route_numpy_ms'] = round(float(np.median([b for _, b in host_t])), 2)
    if args.parent_lib:                        # this tree's median against the parent's, and the parent's own spread
        for name in ('list_dev', 'list_time', 'fill_dev', 'fill_time'):
            t = times[name + '_parent']
            out[name + '_minus_parent_ms'] = round(med[name] - med[name + '_parent'], 4)
            out[name + '_parent_spread_ms'] = round(max(t) - min(t), 4)
            out[name + '_within_parent_spread'] = bool(abs(med[name] - med[name + '_parent']) <= max(t) - min(t))
    out.update(ring_out)
    out['checks'] = check
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    for c in ctx.values():
        c.set_stream(None)
        c.close()
    return 0 if all(v for v in check.values() if isinstance(v, bool)) else 1


if __name__ == '__main__':
    sys.exit(main())
