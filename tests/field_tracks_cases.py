"""The inputs and references of the one-track-per-race tests (tests/test_field_tracks_cpu.py, tests/test_gpu_field_tracks.py): races drawn per
layout by the draws of the one-track suites (test_gpu_field.draw, test_gpu_mixed.draw -- their constructed races 0 .. 3 and the drawn ones, all
already redrawn away from the thresholds of THEIR OWN track), interleaved over the four layouts of plant_tracks_ref.track_set(), and the numpy
models (field_model, mixed_model) called per track subset with that track's own table and lap length.  No GPU, no library."""
import functools

import numpy as np

import field_model as fm
import mixed_model as mm
import plant_tracks_ref as ref
import test_gpu_field as tf
import test_gpu_mixed as tm

# (C, R): a full block of 256 // C races and a partial last block whose races mix tracks
SHAPES = {1: 259, 3: 87, 7: 38}
HORIZONS = (10, 24)
N_MIXED = 10


def ids(R, n_tracks=4):
    """race_track = r % n_tracks: every block holds every track."""
    return (np.arange(R) % n_tracks).astype(np.int32)


def _interleave(parts, race_track):
    """parts[t]: array [R_t, ...] of the races of track t in their order; -> [R, ...] with race r = the (r's rank among track t's races)-th."""
    out = np.empty((len(race_track),) + parts[0].shape[1:], dtype=parts[0].dtype)
    for t, p in enumerate(parts):
        out[race_track == t] = p
    return out


@functools.lru_cache(maxsize=None)
def field_case(C, N, R=None):
    """(ts, race_track [R], x [R,C,6], dims [R,C,2]) -- race r is the next race of test_gpu_field.draw on layout r % 4."""
    R = SHAPES[C] if R is None else R
    ts, rt = ref.track_set(), ids(R)
    draws = [tf.draw(name, C, N, 1000 * C + 10 * N + t, R=int((rt == t).sum())) for t, name in enumerate(ref.NAMES)]
    for t, d in enumerate(draws):
        assert d[0].shape[0] == ts.n_seg[t] and d[1] == ts.lap_length[t]
    return ts, rt, _interleave([d[2] for d in draws], rt), _interleave([d[3] for d in draws], rt)


def field_model(ts, race_track, x, N, dims=None, laps=None):
    """field_model.prep on each track's races with the track's own table and lap length (laps [n_tracks]: other lap lengths for the fold,
    the window, the lap offset, the wrap and `clear` -- the wrong-lap sensitivity check), scattered back to the launch's order."""
    laps = ts.lap_length if laps is None else laps
    parts = [fm.prep(ts.table(t), float(laps[t]), x[race_track == t], N, car_dims=None if dims is None else dims[race_track == t])
             for t in range(ts.n_tracks)]
    return {k: _interleave([p[k] for p in parts], race_track) for k in parts[0]}


@functools.lru_cache(maxsize=None)
def mixed_case(C, N_ilqr, R=None):
    """(ts, race_track, x, dims, policy [R,C]) from test_gpu_mixed.draw per layout (policies over all six codes, one NaN car per layout)."""
    R = SHAPES[C] if R is None else R
    ts, rt = ref.track_set(), ids(R)
    draws = [tm.draw(name, C, N_MIXED, N_ilqr, 2000 * C + N_ilqr + t, R=int((rt == t).sum())) for t, name in enumerate(ref.NAMES)]
    x, dims, pol = (_interleave([d[i] for d in draws], rt) for i in (2, 3, 4))
    assert set(np.unique(pol)) == set(range(mm.N_POLICY)) and np.isnan(x).any()
    return ts, rt, x, dims, pol


def mixed_model(ts, race_track, x, pol, N_ilqr, mode, dims=None):
    """mixed_model.prep on each track's races with the track's own table and lap length, scattered back."""
    parts = [mm.prep(ts.table(t), float(ts.lap_length[t]), x[race_track == t], pol[race_track == t], N_MIXED, N_ilqr, mode,
                     car_dims=None if dims is None else dims[race_track == t]) for t in range(ts.n_tracks)]
    return {k: _interleave([p[k] for p in parts], race_track) for k in parts[0]}
