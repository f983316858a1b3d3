"""Batched closed-loop races, device-resident from the first step to the last.

`mpccbf_races` is the simulation loop of the reference's MPC-CBF racing scenario
(tests/auto_mpccbf_test.py:9-46 -> racing/offboard.py:114-131 -> utils/base.py:780-794) for B independent
races at once: per control step, obstacle predictions of the scripted cars (utils/base.py:879-886), the
window filter and lap offsets of control.mpccbf (control/control.py:499-523,538-540), crx_cbf_prep_dev), ONE crx_cbf_solve_dev over all races, ONE crx_plant_step_wrap_dev incl. the lap
bookkeeping (utils/base.py:795-819).  Three libcrx launches per control step, nothing returns to the host
inside the loop; torch only owns the device memory.

The reference runs such sweeps one race at a time (car_racing/tests/overtake_planner_test.py
--multi-tests); this is the same experiment with the race index as the batch dimension.

Every loop steps its plant through _Plant._advance, the learning-MPC step is LmpcLaps._plan / _apply (GameLaps drives its
`lm` through them), and the run-to-the-end functions share _run_and_log.  The launch sequence of each step() is stated in its
docstring and pinned by tests/test_montecarlo_sequence_cpu.py.

SeedLaps is what comes before the learning MPC: every car's own PID lap and MPC-LTI lap become its own safe set on the device, and
its lmpc_inputs() are the constructor arguments of LmpcLaps / GameLaps as device tensors (PidLaps -> identify -> SeedLaps -> LmpcLaps |
GameLaps runs a fleet from standstill to racing without a host array in between).

FieldGames is GameLaps for a field: every car of a race plays the racing game and is a vehicle of the others (its first launch is
crx_field_traffic_dev); grid_start() is what puts several learning-MPC cars on one track: PidLaps -> identify -> SeedLaps -> grid_start ->
FieldGames.

MixedRaces is the field whose cars differ in controller: a policy code per car (none, pid, lqr, mpc_lti, mpccbf, ilqr), one prep launch
for all of them (crx_mixed_prep_dev), the two solver launches under masks, one commit launch that applies each car's own law.

What the loops are run for -- contacts, cars off the track, lap times, overtakes -- is RaceStats (end of this module): per-car
statistics on the device, one launch per sample, attached to any loop through the loop's stats_inputs().
"""
import numpy as np
import torch

from . import abi, torch_api

_LAP_TRUNC = torch.trunc


class _Noise:
    """The plant's process noise (utils/base.py:929-939) for the batched loops: standard-normal draws from a torch generator
    on the device, one [B, 3] tensor per control step; clipping and scaling happen in crx_plant_step_noise_dev.  seed None =
    zero noise (the `--zero-noise` runs of the reference's scripts; the reference's default is noise ON)."""

    def __init__(self, seed, device):
        self.gen = None
        if seed is not None:
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(int(seed))
        self.device = device

    def draw(self, batch):
        if self.gen is None:
            return None
        return torch.randn((batch, 3), generator=self.gen, dtype=torch.float64, device=self.device)


def _dev(a, dev, dtype=torch.float64, clone=False):
    """Host array -> contiguous tensor of `dtype` on `dev`.  clone: the loop writes to it, so it must own its memory (on the CPU
    torch.as_tensor shares the caller's array).  A tensor (what SeedLaps.lmpc_inputs() hands over) is cast, moved and made contiguous
    without passing through the host, and cloned when asked."""
    if torch.is_tensor(a):
        t = a.to(dtype=dtype, device=dev).contiguous()
        return t.clone() if clone else t
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    return t.clone() if clone else t


def _per_race(v, batch, dev):
    """[batch] float64 on `dev` from a scalar or one value per race."""
    return _dev(np.broadcast_to(np.asarray(v, dtype=float), (batch,)).copy(), dev)


def _models(A, B, batch, dev):
    """(A [batch,6,6], B [batch,6,2]) contiguous float64 on `dev` from one model (6,6), (6,2) or per-problem models, host arrays
    or device tensors (as PidLaps.identify() returns them)."""
    A, B = (m.to(dtype=torch.float64, device=dev) if torch.is_tensor(m) else _dev(m, dev) for m in (A, B))
    if A.dim() == 2 and B.dim() == 2:
        A, B = A.expand(batch, 6, 6), B.expand(batch, 6, 2)
    if tuple(A.shape) != (batch, 6, 6) or tuple(B.shape) != (batch, 6, 2):
        raise ValueError("models: expected shapes %s and %s, got %s and %s" % ((batch, 6, 6), (batch, 6, 2), tuple(A.shape), tuple(B.shape)))
    return A.contiguous(), B.contiguous()


def _order(obj, iters, active=None):
    """Dispatch order of the next solver launch (include/crx.h, "Dispatch order"): obj.dispatch = "longest_first" lists the races
    whose previous solve took most iterations first (and the masked-out ones last); "index" (default) = launch order."""
    if getattr(obj, "dispatch", "index") != "longest_first":
        return None
    return torch_api.longest_first(iters, active)


class Snapshot:
    """The state of a closed-loop object (MpccbfRaces / LmpcLaps / GameLaps, or a Concurrent of them) at this moment: every tensor
    and every plain number reachable through its attributes (workspaces and nested loops included) is copied; restore() puts the
    values AND the attribute bindings back (step() swaps xc / xc_next); tensors held in lists, tuples and dicts and the state of torch.Generator
    objects (the plant-noise stream) are captured too [r6]; objects without a __dict__ hold nothing that is captured.  bench.py uses it to start the timed steps of the closed-loop
    workloads at a stated lap phase whatever --steps / --warmup are.  The caller synchronises the device around both calls."""

    def __init__(self, obj):
        import ctypes
        self.tensors, self.scalars, self.items, self.gens = [], [], [], []
        seen = set()
        skip = (ctypes.Structure, torch.cuda.Stream, type)

        def visit(holder, key, v, is_item):
            """one value reachable from `obj`: holder.key (attribute) or holder[key] (list / dict item)"""
            if torch.is_tensor(v):
                (self.items if is_item else self.tensors).append((holder, key, v, v.clone()))
            elif isinstance(v, torch.Generator):
                self.gens.append((v, v.get_state()))          # the plant-noise stream restarts where it was
            elif isinstance(v, (bool, int, float)):
                if not is_item:
                    self.scalars.append((holder, key, v))
            elif isinstance(v, (list, tuple)):
                if id(v) not in seen:
                    seen.add(id(v))
                    for i, e in enumerate(v):
                        visit(v, i, e, True)
            elif isinstance(v, dict):
                if id(v) not in seen:
                    seen.add(id(v))
                    for k2, e in list(v.items()):
                        visit(v, k2, e, True)
            elif hasattr(v, "__dict__") and not isinstance(v, skip):
                walk(v)

        def walk(o):
            if id(o) in seen or not hasattr(o, "__dict__"):      # (objects with __slots__ only: nothing to capture)
                return
            seen.add(id(o))
            for k, v in list(vars(o).items()):
                visit(o, k, v, False)

        walk(obj)

    def restore(self):
        for o, k, t, c in self.tensors:
            t.copy_(c)
            setattr(o, k, t)
        for holder, k, t, c in self.items:             # tensors held in lists / dicts: values back; a mutable holder also gets its binding back
            t.copy_(c)
            if not isinstance(holder, tuple):
                holder[k] = t
        for o, k, v in self.scalars:
            setattr(o, k, v)
        for gen, state in self.gens:
            gen.set_state(state)


class Concurrent:
    """K independent sub-batches of races stepping on K HIP streams.  Races do not interact, so a batch can be cut anywhere; what
    the cut buys is OVERLAP: the streams free-run (no join per step), a sub-batch's plant (100 serial Euler sub-steps per vehicle:
    ~0.2 ms on 64 wavefronts, 6 % of the chip) and the straggler tail of its solver launch run while the next sub-batch's solver
    launch occupies the other CUs.  Every race computes exactly what it computes in one big batch (bit-identical).  `parts` are
    MpccbfRaces / LmpcLaps / GameLaps objects over disjoint slices of the races; step() issues one control step of every part and
    returns without waiting; call torch.cuda.synchronize() (or sync()) before reading results.
    Streams only overlap when they sit on different HARDWARE queues: the HIP runtime multiplexes a process's streams onto
    GPU_MAX_HW_QUEUES of them (default 4) and streams sharing one serialise -- two sub-batches on one queue are SLOWER than one
    batch.  Which streams share is not ours to choose and, with torch's stream pool, depended on how many streams the process
    had handed out before (3.24 .. 5.6 ms per racing-game step: tools/stream_offset_probe.py), so the streams are libcrx's:
    crx_streams_create measures which of its candidates overlap and returns a set that does (include/crx.h "Streams").  Two
    sub-batches of GameLaps want six (one each + the two branch streams of each): set GPU_MAX_HW_QUEUES=8 in the environment
    before the runtime initialises (bench.py does); with fewer queues than that the parts run their branches one after the
    other on their sub-batch stream.  Measured, 4096 races per step (tools/gpu_round3_i.sh): races 0.784 -> 0.687 ms,
    learning-MPC laps 3.82 -> 3.31 ms, racing game 3.56 -> 3.25 ms with two sub-batches and 8 queues."""

    def __init__(self, parts, device=None, streams=None):
        self.parts = list(parts)
        dev = torch.device(device if device is not None else "cuda")
        self.device = dev
        K = len(self.parts)
        inner = [p for p in self.parts if hasattr(p, "set_branch_streams")]
        if streams is not None:            # the caller's streams (K, or K + 2 per GameLaps part), taken as they are
            self.n_concurrent = len(streams)
        else:
            streams, self.n_concurrent = torch_api.new_streams(K + 2 * len(inner), dev)   # the first n_concurrent overlap pairwise
        self.streams = streams[:K]
        for i, part in enumerate(inner):
            if K == 1 or self.n_concurrent >= K + 2 * len(inner):
                part.set_branch_streams(streams[K + 2 * i], streams[K + 2 * i + 1])
            else:                          # not enough hardware queues for nested streams: branches in sequence on the part's stream
                part.overlap = False
        cur = torch.cuda.current_stream(dev)
        for st in self.streams:            # whatever set the parts up on the caller's stream comes first
            st.wait_stream(cur)

    def step(self):
        for part, st in zip(self.parts, self.streams):
            with torch.cuda.stream(st):
                part.step()

    def sync(self):
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            cur.wait_stream(st)

    def cat(self, get):
        """Concatenate a per-race tensor of every part (after sync()): get(part) -> tensor [B_part, ...]."""
        self.sync()
        return torch.cat([get(p) for p in self.parts], dim=0)


class _Plant:
    """The plant side of a closed loop, held by the loop object itself: the cars' states xc (curvilinear) / xg (global) [B,6], the
    buffers xc_next / xg_next the next plant launch writes, the lap counters, the track table, the plant descriptor and the
    process noise, and plant_params: one parameter set per car [B,10], or None.  _advance() is the one place a loop steps its plant.  The contract bench.py times the solver launches by:
    after a step, xc_next is the state that step's solver launch was built for."""

    def _plant_init(self, track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params=None, tracks=None, track_id=None,
                    track_set=None):
        dev = torch.device(device if device is not None else "cuda")
        self.device, self.lap_length, self.timestep = dev, lap_length, timestep
        self.noise = _Noise(noise_seed, dev)
        self.xc, self.xg = _dev(xcurv0, dev, clone=True), _dev(xglob0, dev, clone=True)
        self.xc_next, self.xg_next = torch.empty_like(self.xc), torch.empty_like(self.xg)
        self.batch = self.xc.shape[0]
        self.laps = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        # tracks (abi.track_set) and track_id [B], host array or device tensor: car b on track track_id[b] (crx_plant_step_tracks_dev);
        # track_table and lap_length are then unused (None), self.lap_length is the per-car tensor lap_length[track_id] and the plant
        # descriptor carries track 0's row count and lap length only to be a valid one.  None: the one track_table for all cars.
        # track_set: the same, already on the device (a field's RaceTrackSetDev: the cars' ids made of the races')
        self.tracks = None
        if (tracks is None) != (track_id is None):
            raise ValueError("tracks and track_id go together: a track set and every car's track, or neither")
        if track_set is not None:
            tracks = track_set.host
        if tracks is not None:
            if track_table is not None or lap_length is not None:
                raise ValueError("with tracks= the loop has no track_table / lap_length of its own: pass None for both")
            self.tracks = track_set if track_set is not None else torch_api.TrackSetDev(tracks, track_id, dev)
            if tuple(self.tracks.track_id.shape) != (self.batch,):
                raise ValueError("track_id: expected shape %s, got %s" % ((self.batch,), tuple(self.tracks.track_id.shape)))
            self.lap_length = self.tracks.car_lap
            self.tab = self.tracks.tracks
            self.plant = abi.plant_desc(int(tracks.n_seg[0]), float(tracks.lap_length[0]), timestep=timestep)
        else:
            self.tab = _dev(track_table, dev)
            self.plant = abi.plant_desc(self.tab.shape[0], lap_length, timestep=timestep)
        # plant_params [B,10] (abi.plant_params, synth.fleet_plant_params), host array or device tensor: every car its own BicycleDynamicsParam
        # set (crx_plant_step_params_dev).  None: the one set of self.plant for all of them
        self.plant_params = None
        if plant_params is not None:
            P = plant_params.to(dtype=torch.float64, device=dev) if torch.is_tensor(plant_params) else _dev(plant_params, dev)
            if tuple(P.shape) != (self.batch, abi.CRX_PLANT_NPARAM):
                raise ValueError("plant_params: expected shape %s, got %s" % ((self.batch, abi.CRX_PLANT_NPARAM), tuple(P.shape)))
            self.plant_params = P.contiguous()
        return dev

    def _advance(self, u, u_stride, noise_z=None):
        """ONE crx_plant_step_wrap_dev (plant + lap bookkeeping) with race b's input at u[b * u_stride], then xc / xc_next and
        xg / xg_next exchange bindings.  noise_z None: the step's draws come from the loop's generator, which a given noise_z
        leaves alone."""
        if noise_z is None:
            noise_z = self.noise.draw(self.batch)
        if self.tracks is not None:
            torch_api.plant_step_tracks_wrap_dev(self.plant, self.tracks, self.xg, self.xc, u, u_stride, self.xg_next, self.xc_next, self.laps,
                                                 noise_z=noise_z, params=self.plant_params)
        else:
            torch_api.plant_step_wrap_dev(self.plant, self.tab, self.xg, self.xc, u, u_stride, self.xg_next, self.xc_next, self.laps,
                                          noise_z=noise_z, params=self.plant_params)
        self.xg, self.xg_next = self.xg_next, self.xg
        self.xc, self.xc_next = self.xc_next, self.xc

    def stats_inputs(self, **more):
        """What RaceStats samples, read at call time (xc and xc_next exchange bindings every step): the cars' states and lap counters,
        the clock of the scripted cars, the track, the speed targets; the loops add their opponents (scripted: car_s0, car_v, car_ey
        [B,V]; a field: n_cars, car_dims), a flag [B] int32 and the half-sums of their cars' dimensions where they have them."""
        inp = dict(xcurv=self.xc, laps=self.laps, t=getattr(self, "t", 0.0), lap_length=self.lap_length,
                   track_width=getattr(self, "track_width", None), xt=getattr(self, "xt", None))
        inp.update(more)
        return inp


def _one_track_only(loop, tracks, track_id):
    """The loops whose other launches take ONE track table or ONE lap length (a prep descriptor, a safe set, a scene) refuse a track set."""
    if tracks is not None or track_id is not None:
        raise ValueError("%s runs on one track: tracks= / track_id= (one track per car) are taken by PidLaps, LqrLaps and MpccbfRaces only -- "
                         "its other launches read one track table or one lap length" % loop)


def _race_tracks_only(loop, tracks, track_id, race_track):
    """FieldRaces and MixedRaces: a field's unit is the race, so a track set comes with race_track= (one id per race); the per-car track_id=
    stays refused, and so does a set without race_track=."""
    if track_id is not None:
        _one_track_only(loop, tracks, track_id)
    if (tracks is None) != (race_track is None):
        raise ValueError("%s: tracks= and race_track= go together: a track set (abi.track_set) and every race's track [R], or neither" % loop)


def _run_and_log(step, steps, log_every, getters, before=()):
    """`steps` calls of step(); at every log_every-th one, a clone of what each getter (name -> callable returning a device tensor)
    returns after the step -- the names in `before` are read ahead of that step instead -- and "xcurv" once more at the start.
    Returns name -> host array with the logged step as the first dimension."""
    logs = {name: [] for name in getters}
    logs["xcurv"].append(getters["xcurv"]().clone())
    for k in range(steps):
        logged = (k + 1) % log_every == 0
        if logged:
            for name in before:
                logs[name].append(getters[name]().clone())
        step()
        if logged:
            for name in getters:
                if name not in before:
                    logs[name].append(getters[name]().clone())
    return {name: torch.stack(rows).cpu().numpy() for name, rows in logs.items()}


class MpccbfRaces(_Plant):
    """State of B races on the device; step() advances all of them by one control step."""

    def __init__(self, track_table, lap_length, track_width, A, B, xcurv0, xglob0, car_s0, car_v, car_ey,
                 vt=0.8, eyt=0.0, N=10, alpha=0.8, timestep=0.1, device=None, noise_seed=None, models=None, plant_params=None, tracks=None,
                 track_id=None):
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params, tracks, track_id)
        f64 = dict(dtype=torch.float64, device=dev)
        self.s0, self.v, self.ey = (_dev(a, dev) for a in (car_s0, car_v, car_ey))
        Bn, V = self.s0.shape
        if V > abi.CRX_MAX_OBS:
            raise ValueError("at most %d scripted cars" % abi.CRX_MAX_OBS)
        self.N, self.V, self.track_width = N, V, track_width
        self.desc = abi.cbf_desc(N, V, A, B, alpha=alpha, margin=0.2, ey_max=track_width)
        self.xt = torch.tensor([vt, 0, 0, 0, 0, eyt], **f64).repeat(Bn, 1).contiguous()
        self.ws = torch_api.CbfWorkspace(self.desc, Bn, dev)
        # models = (A [B,6,6], B [B,6,2]), host arrays or device tensors (PidLaps.identify()): every race's controller on its own model
        # (crx_cbf_solve_models_dev); A, B above are then unused.  The reach table is computed here, once
        self.models = None if models is None else torch_api.CbfModels(self.desc, *_models(models[0], models[1], Bn, dev))
        self.jdt = torch.arange(N + 1, **f64) * timestep
        self.ar = torch.arange(V, device=dev)
        self.obs_s = torch.empty((Bn, V, N + 1), **f64)
        self.obs_e = torch.empty((Bn, V, N + 1), **f64)
        self.lap_off = torch.empty((Bn, V), **f64)
        self.n_obs = torch.empty((Bn,), dtype=torch.int32, device=dev)
        self.t = 0.0   # every vehicle's own clock, advanced by `+= timestep` like the reference's (base.py:889,941)
        self.u = None

    def step(self):
        """One control step of every race, three libcrx launches and nothing else: cbf_prep_dev, cbf_solve_dev,
        plant_step_wrap_dev (dispatch = "longest_first": one longest_first ahead of the solver launch).  On a track set: cbf_prep_laps_dev
        (every race folded by its own lap length), cbf_solve_dev, plant_step_tracks_wrap_dev."""
        N = self.N
        prep = torch_api.cbf_prep_dev if self.tracks is None else torch_api.cbf_prep_laps_dev
        prep(N, self.lap_length, self.t, self.timestep, self.xc, self.s0, self.v, self.ey, self.obs_s, self.obs_e, self.lap_off, self.n_obs)
        torch_api.cbf_solve_dev(self.desc, self.xc, self.xt, self.obs_s, self.obs_e, self.lap_off, self.n_obs, ws=self.ws,
                                order=_order(self, self.ws.iters), models=self.models)
        self._advance(self.ws.U, 2 * N)   # the plant reads u_0 of every race straight out of the solver's U [B][N][2]
        self.u = self.ws.U[:, 0, :]
        self.t += self.timestep

    def stats_inputs(self):
        return super().stats_inputs(car_s0=self.s0, car_v=self.v, car_ey=self.ey)

    def step_glue(self):
        """The same control step with the prediction / window filter / packing / lap wrap written as element-wise
        torch ops (the first version; kept as an independent restatement for the tests)."""
        N, xc = self.N, self.xc
        L = self.lap_length if self.tracks is None else self.lap_length[:, None]     # a track set: every race's own, [B,1]
        tt = self.t + self.jdt                                                       # [N+1]
        obs_s = self.v[:, :, None] * tt[None, None, :] + self.s0[:, :, None]         # [B,V,N+1]
        obs_e = self.ey[:, :, None] + 0.0 * tt[None, None, :]
        margin = 2.0 * xc[:, 0:1]
        nce = _LAP_TRUNC(xc[:, 4:5] / L)
        dist_ego = xc[:, 4:5] - nce * L
        nco = _LAP_TRUNC(obs_s[:, :, 0] / L)
        dist_obs = obs_s[:, :, 0] - nco * L
        keep = (dist_ego > dist_obs - margin) & (dist_ego < dist_obs + margin)       # [B,V]
        lap_off = (nce - nco) * L
        order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
        n_obs = keep.sum(dim=1).to(torch.int32)
        live = (self.ar[None, :] < n_obs[:, None])
        ps = torch.gather(obs_s, 1, order[:, :, None].expand(-1, -1, N + 1)) * live[:, :, None]
        pe = torch.gather(obs_e, 1, order[:, :, None].expand(-1, -1, N + 1)) * live[:, :, None]
        po = torch.gather(lap_off, 1, order) * live
        torch_api.cbf_solve_dev(self.desc, xc, self.xt, ps.contiguous(), pe.contiguous(), po.contiguous(), n_obs.contiguous(),
                                ws=self.ws, models=self.models)
        self.u = self.ws.U[:, 0, :].contiguous()
        if self.tracks is None:
            self.xg, xc = torch_api.plant_step_dev(self.plant, self.tab, self.xg, xc, self.u, params=self.plant_params)
        else:
            self.xg, xc = torch_api.plant_step_tracks_dev(self.plant, self.tracks, self.xg, xc, self.u, params=self.plant_params)
        crossed = xc[:, 4] > self.lap_length
        xc[:, 4] = torch.where(crossed, xc[:, 4] - self.lap_length, xc[:, 4])
        self.laps += crossed.to(torch.int32)
        self.xc = xc
        self.t += self.timestep


def mpccbf_races(track_table, lap_length, track_width, A, B, xcurv0, xglob0, car_s0, car_v, car_ey, steps,
                 vt=0.8, eyt=0.0, N=10, alpha=0.8, timestep=0.1, device=None, log_every=1, glue=False, models=None, plant_params=None,
                 tracks=None, track_id=None):
    """xcurv0, xglob0 [B,6]; car_s0, car_v, car_ey [B,V] with V <= 3: scripted cars s(t) = v t + s0, ey(t) = ey
    (NoDynamicsModel, utils/base.py:847-890); models = (A [B,6,6], B [B,6,2]): one controller model per race; plant_params [B,10]: one car per race.  Returns host arrays: xcurv [T+1,B,6] (T = steps/log_every), u [T,B,2],
    status [T,B], laps [B].  tracks (abi.track_set), track_id [B]: race b on its own track (track_table and lap_length None)."""
    r = MpccbfRaces(track_table, lap_length, track_width, A, B, xcurv0, xglob0, car_s0, car_v, car_ey, vt=vt, eyt=eyt,
                    N=N, alpha=alpha, timestep=timestep, device=device, models=models, plant_params=plant_params, tracks=tracks,
                    track_id=track_id)
    logs = _run_and_log(r.step_glue if glue else r.step, steps, log_every,
                        dict(xcurv=lambda: r.xc, u=lambda: r.u, status=lambda: r.ws.status))
    return dict(logs, laps=r.laps.cpu().numpy())


class _Field(_Plant):
    """What FieldRaces and MixedRaces share: R races of C cars, the plant batch R*C race-major and car-minor; xt [R*C,6], the cars' targets;
    min_clear [R*C]: each car's smallest super-ellipse value against the cars of its race over the states the steps so far STARTED from
    (below 1: contact); fd: the loop's field or mixed descriptor, for its l_sum, w_sum."""

    def _field_init(self, track_table, lap_length, track_width, timestep, xcurv0, xglob0, n_cars, vt, eyt, N, car_dims, noise_seed, device,
                    plant_params, n_races=None, tracks=None, race_track=None):
        """n_races: the races the caller's other arguments make (MixedRaces' policy); None: as many as xcurv0 holds.  tracks (abi.track_set)
        and race_track [R], integer, host array or tensor: race r on track race_track[r], all its cars on it -- track_table and lap_length are
        then None, self.tracks is a torch_api.RaceTrackSetDev (the plant steps through its tracks entry with track_id = race_track repeated
        n_cars times), self.lap_length the cars' own lap lengths [R*C], and _prep_geometry() gives the prep descriptors track 0's row count
        and lap length only to make them valid ones.  One track_width serves all tracks.  Returns the device."""
        Cn = int(n_cars)
        if not 1 <= Cn <= abi.CRX_MAX_OBS + 1:
            raise ValueError("1 .. %d cars per race" % (abi.CRX_MAX_OBS + 1))
        x0, g0 = (np.asarray(a, dtype=float).reshape(-1, 6) for a in (xcurv0, xglob0))   # [R*C,6] or [R,C,6]
        R = x0.shape[0] // Cn if n_races is None else n_races
        if x0.shape[0] != R * Cn or g0.shape != x0.shape:
            raise ValueError("xcurv0, xglob0: %d and %d cars" % (x0.shape[0], g0.shape[0])
                             + (" do not make races of %d" % Cn if n_races is None else ", policy has %d x %d" % (R, Cn)))
        ts = None
        if tracks is not None:
            ts = torch_api.RaceTrackSetDev(tracks, race_track, Cn, torch.device(device if device is not None else "cuda"))
            if tuple(ts.race_track.shape) != (R,):
                raise ValueError("race_track: expected shape %s, got %s" % ((R,), tuple(ts.race_track.shape)))
        dev = self._plant_init(track_table, lap_length, timestep, x0, g0, noise_seed, device, plant_params, track_set=ts)
        self.N, self.n_races, self.n_cars, self.track_width = N, R, Cn, track_width
        # vt, eyt: scalars or one value per car [R,C] -- different target speeds are what makes the cars meet
        xt = np.zeros((self.batch, 6))
        xt[:, 0] = np.broadcast_to(np.asarray(vt, dtype=float), (R, Cn)).reshape(-1)
        xt[:, 5] = np.broadcast_to(np.asarray(eyt, dtype=float), (R, Cn)).reshape(-1)
        self.xt = _dev(xt, dev)
        # car_dims [R,C,2]: (length, width) of every car; None: the descriptor's l_sum, w_sum for every pair
        self.car_dims = None if car_dims is None else _dev(np.asarray(car_dims, dtype=float).reshape(R, Cn, 2), dev)
        self.min_clear = torch.full((self.batch,), float("inf"), dtype=torch.float64, device=dev)
        return dev

    def _prep_geometry(self):
        """(n_seg, lap_length) of the loop's prep descriptor: the one track's, or track 0's of a set (unused by the `tracks` entries)."""
        if self.tracks is not None:
            return int(self.tracks.host.n_seg[0]), float(self.tracks.host.lap_length[0])
        return self.tab.shape[0], self.lap_length

    def _join_clear(self, clear):
        torch.minimum(self.min_clear, clear, out=self.min_clear)

    def stats_inputs(self):
        return super().stats_inputs(n_cars=self.n_cars, car_dims=self.car_dims, l_sum=self.fd.l_sum, w_sum=self.fd.w_sum)


class FieldRaces(_Field):
    """R races of C cars that ALL drive themselves under MPC-CBF: every car is the ego of its own NLP and an obstacle of the C - 1
    others, predicted by the zero-input roll-out of the reference's driven model (racing/offboard.py:51-94) as control.mpccbf consumes it
    with realtime_flag == True (control/control.py:512-514).  The plant batch is R*C, race-major, car-minor; all cars of a step see
    the states at the start of the step (include/crx.h, crx_field_prep_dev, quirks F1-F7).  min_clear [R*C]: see _Field."""

    def __init__(self, track_table, lap_length, track_width, A, B, xcurv0, xglob0, n_cars, vt=0.8, eyt=0.0, N=10, alpha=0.8, timestep=0.1,
                 device=None, noise_seed=None, models=None, plant_params=None, car_dims=None, tracks=None, track_id=None, race_track=None):
        _race_tracks_only("FieldRaces", tracks, track_id, race_track)
        dev = self._field_init(track_table, lap_length, track_width, timestep, xcurv0, xglob0, n_cars, vt, eyt, N, car_dims, noise_seed,
                               device, plant_params, tracks=tracks, race_track=race_track)
        Bn, R, Cn = self.batch, self.n_races, self.n_cars
        self.desc = abi.cbf_desc(N, Cn - 1, A, B, alpha=alpha, margin=0.2, ey_max=track_width)
        self.fdesc = self.fd = abi.field_desc(N, Cn, *self._prep_geometry(), dt=timestep)
        self.ws = torch_api.CbfWorkspace(self.desc, Bn, dev)
        # models = (A [R*C,6,6], B [R*C,6,2]): every car's controller on its own model, as in MpccbfRaces
        self.models = None if models is None else torch_api.CbfModels(self.desc, *_models(models[0], models[1], Bn, dev))
        self.fws = torch_api.FieldWorkspace(self.fdesc, R, dev, dims=car_dims is not None)
        self.u = None

    def step(self):
        """One control step of every car of every race, three libcrx launches: field_prep_dev, cbf_solve_dev, plant_step_wrap_dev
        (dispatch = "longest_first": one longest_first ahead of the solver launch); then `clear` joins the running minimum.  With
        tracks= / race_track=: field_prep_tracks_dev, cbf_solve_dev, plant_step_tracks_wrap_dev."""
        f = self.fws
        if self.tracks is None:
            torch_api.field_prep_dev(self.fdesc, self.tab, self.xc, f, car_dims=self.car_dims)
        else:
            torch_api.field_prep_tracks_dev(self.fdesc, self.tracks, self.xc, f, car_dims=self.car_dims)
        torch_api.cbf_solve_dev(self.desc, self.xc, self.xt, f.obs_s, f.obs_ey, f.lap_off, f.n_obs, ws=self.ws,
                                order=_order(self, self.ws.iters), models=self.models, obs_dims=f.obs_dims)
        self._advance(self.ws.U, 2 * self.N)
        self.u = self.ws.U[:, 0, :]
        self._join_clear(f.clear)


def field_races(track_table, lap_length, track_width, A, B, xcurv0, xglob0, n_cars, steps, vt=0.8, eyt=0.0, N=10, alpha=0.8, timestep=0.1,
                device=None, log_every=1, noise_seed=None, models=None, plant_params=None, car_dims=None, tracks=None, race_track=None):
    """xcurv0, xglob0 [R*C,6] or [R,C,6]; vt, eyt scalars or [R,C]; models = (A [R*C,6,6], B [R*C,6,2]); plant_params [R*C,10]; car_dims
    [R,C,2].  Returns host arrays: xcurv [T+1,R*C,6] (T = steps / log_every), u [T,R*C,2], status, iters, n_obs [T,R*C], laps [R*C],
    min_clear [R*C].  tracks (abi.track_set), race_track [R]: race r on its own track (track_table and lap_length None)."""
    r = FieldRaces(track_table, lap_length, track_width, A, B, xcurv0, xglob0, n_cars, vt=vt, eyt=eyt, N=N, alpha=alpha, timestep=timestep,
                   device=device, noise_seed=noise_seed, models=models, plant_params=plant_params, car_dims=car_dims, tracks=tracks,
                   race_track=race_track)
    logs = _run_and_log(r.step, steps, log_every, dict(xcurv=lambda: r.xc, u=lambda: r.u, status=lambda: r.ws.status,
                                                       iters=lambda: r.ws.iters, n_obs=lambda: r.fws.n_obs))
    return dict(logs, laps=r.laps.cpu().numpy(), min_clear=r.min_clear.cpu().numpy())


class MixedRaces(_Field):
    """R races of C cars, every car under its OWN controller, as the reference's simulator holds its vehicles (CarRacingSim.add_vehicle +
    ModelBase.set_ctrl_policy, racing/offboard.py:14-45; sim() steps them together, :114-131): policy [R,C] of abi.POLICY_* codes or names
    ("none", "pid", "lqr", "mpc_lti", "mpccbf", "ilqr").  The plant batch is R*C, race-major, car-minor; all cars of a step see the states at
    the start of the step (include/crx.h "Mixed fields", quirks F1-F3, F6, M1, M2).  One NLP launch serves the mpc_lti and mpccbf cars (they
    share Q and R; an mpc_lti car has no obstacles), one iLQR launch the ilqr cars, each under its mask; a launch whose policy no car has
    is not issued -- decided here, from the host `policy`.  status [R*C]: the solve's status for the solver policies, CRX_CONVERGED for pid
    and lqr, CRX_SKIPPED for none.  min_clear [R*C] as in FieldRaces."""

    def __init__(self, track_table, lap_length, track_width, A, B, xcurv0, xglob0, policy, vt=0.8, eyt=0.0, N=10, ilqr_N=50, ilqr_max_iter=150,
                 ilqr_obstacles=0, alpha=0.8, timestep=0.1, device=None, noise_seed=None, models=None, plant_params=None, car_dims=None,
                 tracks=None, track_id=None, race_track=None):
        _race_tracks_only("MixedRaces", tracks, track_id, race_track)
        pol = abi.policy_codes(policy)
        if pol.ndim != 2 or not 1 <= pol.shape[1] <= abi.CRX_MAX_OBS + 1:
            raise ValueError("policy: [R,C] with 1 .. %d cars per race" % (abi.CRX_MAX_OBS + 1))
        R, Cn = pol.shape
        # xt is the target of the NLP, iLQR and LQR cars, (vt, eyt) the PID cars'
        dev = self._field_init(track_table, lap_length, track_width, timestep, xcurv0, xglob0, Cn, vt, eyt, N, car_dims, noise_seed, device,
                               plant_params, n_races=R, tracks=tracks, race_track=race_track)
        Bn = self.batch
        has = lambda *codes: bool(np.isin(pol, codes).any())   # noqa: E731
        has_nlp, has_ilqr, has_lqr, has_pid = has(abi.POLICY_MPC_LTI, abi.POLICY_MPCCBF), has(abi.POLICY_ILQR), has(abi.POLICY_LQR), has(abi.POLICY_PID)
        self.policy = _dev(pol.reshape(-1), dev, dtype=torch.int32)
        self.mdesc = self.fd = abi.mixed_desc(N, ilqr_N if has_ilqr else 0, Cn, *self._prep_geometry(), ilqr_obstacles=ilqr_obstacles, dt=timestep)
        self.vt, self.eyt = (self.xt[:, 0].contiguous(), self.xt[:, 5].contiguous()) if has_pid else (None, None)
        # models = (A [R*C,6,6], B [R*C,6,2]): every car's controller on its own model -- the NLP's, the iLQR's and the LQR design's
        mAB = None if models is None else _models(models[0], models[1], Bn, dev)
        self.desc = self.ws = self.models = None
        if has_nlp:
            self.desc = abi.cbf_desc(N, Cn - 1, A, B, alpha=alpha, margin=0.2, ey_max=track_width)
            self.ws = torch_api.CbfWorkspace(self.desc, Bn, dev)
            self.models = None if mAB is None else torch_api.CbfModels(self.desc, *mAB)
        self.idesc = self.iws = self.ilqr_models = None
        if has_ilqr:
            self.idesc = abi.ilqr_desc(ilqr_N, A, B, max_iter=ilqr_max_iter, n_obs_max=Cn - 1, l_sum=self.mdesc.l_sum, w_sum=self.mdesc.w_sum)
            self.iws = torch_api.IlqrWorkspace(self.idesc, Bn, dev)
            self.ilqr_models = mAB
        self.K = None
        if has_lqr:   # one design launch, here: the LQR cars' gains (the other cars' rows stay zero)
            m_lqr = _dev((pol.reshape(-1) == abi.POLICY_LQR).astype(np.int32), dev, dtype=torch.int32)
            self.K = torch_api.lqr_design_dev(abi.lqr_desc(), *(mAB if mAB is not None else _models(A, B, Bn, dev)), active=m_lqr).K
        # car_dims serves the NLP family and `clear` (M2)
        self.mws = torch_api.MixedWorkspace(self.mdesc, R, dev, dims=car_dims is not None)
        self.u = torch.zeros((Bn, 2), dtype=torch.float64, device=dev)
        self.status = torch.zeros(Bn, dtype=torch.int32, device=dev)

    def step(self):
        """One control step of every car of every race: mixed_prep_dev, cbf_solve_dev (active = m_nlp), ilqr_solve_dev (active = m_ilqr),
        mixed_commit_dev, plant_step_wrap_dev -- a solver launch whose policy no car has is left out and its family given as None
        (dispatch = "longest_first": one longest_first ahead of the NLP launch); then `clear` joins the running minimum.  With tracks= /
        race_track=: mixed_prep_tracks_dev in place of mixed_prep_dev and plant_step_tracks_wrap_dev in place of plant_step_wrap_dev."""
        m = self.mws
        if self.tracks is None:
            torch_api.mixed_prep_dev(self.mdesc, self.tab, self.xc, self.policy, m, car_dims=self.car_dims)
        else:
            torch_api.mixed_prep_tracks_dev(self.mdesc, self.tracks, self.xc, self.policy, m, car_dims=self.car_dims)
        if self.ws is not None:
            torch_api.cbf_solve_dev(self.desc, self.xc, self.xt, m.obs_s, m.obs_ey, m.lap_off, m.n_obs, ws=self.ws, active=m.m_nlp,
                                    order=_order(self, self.ws.iters, m.m_nlp), models=self.models, obs_dims=m.obs_dims)
        if self.iws is not None:
            torch_api.ilqr_solve_dev(self.idesc, self.xc, self.xt, m.il_obs_s, m.il_obs_ey, m.il_lap_off, m.il_n_obs, ws=self.iws,
                                     active=m.m_ilqr, models=self.ilqr_models)
        torch_api.mixed_commit_dev(self.policy, self.xc, self.u, self.status,
                                   pid=None if self.vt is None else (self.vt, self.eyt), lqr=None if self.K is None else (self.K, self.xt),
                                   nlp=None if self.ws is None else (self.ws.U, self.ws.status),
                                   ilqr=None if self.iws is None else (self.iws.U, self.iws.status))
        self._advance(self.u, 2)
        self._join_clear(m.clear)


def mixed_races(track_table, lap_length, track_width, A, B, xcurv0, xglob0, policy, steps, vt=0.8, eyt=0.0, N=10, ilqr_N=50, ilqr_max_iter=150,
                ilqr_obstacles=0, alpha=0.8, timestep=0.1, device=None, log_every=1, noise_seed=None, models=None, plant_params=None, car_dims=None,
                tracks=None, race_track=None):
    """policy [R,C] codes or names; xcurv0, xglob0 [R*C,6] or [R,C,6]; vt, eyt scalars or [R,C]; models = (A [R*C,6,6], B [R*C,6,2]);
    plant_params [R*C,10]; car_dims [R,C,2].  Returns host arrays: xcurv [T+1,R*C,6] (T = steps / log_every), u [T,R*C,2], status [T,R*C],
    laps [R*C], min_clear [R*C].  tracks (abi.track_set), race_track [R]: race r on its own track (track_table and lap_length None)."""
    r = MixedRaces(track_table, lap_length, track_width, A, B, xcurv0, xglob0, policy, vt=vt, eyt=eyt, N=N, ilqr_N=ilqr_N, ilqr_max_iter=ilqr_max_iter,
                   ilqr_obstacles=ilqr_obstacles, alpha=alpha, timestep=timestep, device=device, noise_seed=noise_seed, models=models,
                   plant_params=plant_params, car_dims=car_dims, tracks=tracks, race_track=race_track)
    logs = _run_and_log(r.step, steps, log_every, dict(xcurv=lambda: r.xc, u=lambda: r.u, status=lambda: r.status))
    return dict(logs, laps=r.laps.cpu().numpy(), min_clear=r.min_clear.cpu().numpy())


class IlqrRaces(_Plant):
    """B copies of the reference's iLQR racing scenario (car_racing/tests/ilqr_test.py: ego under iLQRRacing, one scripted car
    s(t) = v t + s0, ey(t) = ey), device-resident.  Per control step, without touching the host: the scripted car's N+1
    predictions from its own clock (utils/base.py:879-886; control.ilqr applies no distance window, quirk I1), the lap offset
    (int(s_ego / L) - int(s_obs,0 / L)) L (quirk I5), ONE crx_ilqr_solve_dev over all races, ONE crx_plant_step_wrap_dev."""

    def __init__(self, track_table, lap_length, A, B, xcurv0, xglob0, car_s0, car_v, car_ey, vt=0.8, eyt=0.0, N=50,
                 max_iter=150, timestep=0.1, ego_dims=(0.4, 0.2), car_dims=(0.4, 0.2), device=None, noise_seed=None, models=None,
                 plant_params=None, tracks=None, track_id=None):
        _one_track_only("IlqrRaces", tracks, track_id)
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params)
        f64 = dict(dtype=torch.float64, device=dev)
        self.s0, self.v, self.ey = (_dev(np.asarray(a, dtype=float).reshape(-1, 1), dev) for a in (car_s0, car_v, car_ey))
        self.N, Bn = N, self.batch
        self.desc = abi.ilqr_desc(N, A, B, max_iter=max_iter, n_obs_max=1, l_sum=ego_dims[0] / 2 + car_dims[0] / 2,
                                  w_sum=ego_dims[1] / 2 + car_dims[1] / 2)
        self.xt = torch.tensor([vt, 0, 0, 0, 0, eyt], **f64).repeat(Bn, 1).contiguous()
        self.ws = torch_api.IlqrWorkspace(self.desc, Bn, dev)
        self.jdt = torch.arange(N + 1, **f64) * timestep
        self.n_obs = torch.ones(Bn, dtype=torch.int32, device=dev)
        self.t = 0.0   # the scripted car's clock, advanced by `+= timestep` like the reference's (base.py:889)
        self.u = None
        # models = (A [B,6,6], B [B,6,2]): every race on its own model (crx_ilqr_solve_models_dev); A, B above are then unused
        self.models = None if models is None else _models(models[0], models[1], Bn, dev)

    def predictions(self):
        """(obs_s, obs_ey [B,1,N+1], lap_off [B,1]) of the current step."""
        L = self.lap_length
        tt = self.t + self.jdt                                                  # time + index * delta_t
        obs_s = (self.v * tt[None, :] + self.s0)[:, None, :].contiguous()
        obs_e = (self.ey + 0.0 * tt[None, :])[:, None, :].contiguous()
        lap_off = ((_LAP_TRUNC(self.xc[:, 4:5] / L) - _LAP_TRUNC(obs_s[:, :, 0] / L)) * L).contiguous()
        return obs_s, obs_e, lap_off

    def stats_inputs(self):
        return super().stats_inputs(car_s0=self.s0, car_v=self.v, car_ey=self.ey, l_sum=self.desc.l_sum, w_sum=self.desc.w_sum)

    def step(self):
        """One control step of every race: predictions (torch ops), then ilqr_solve_dev, plant_step_wrap_dev."""
        obs_s, obs_e, lap_off = self.predictions()
        torch_api.ilqr_solve_dev(self.desc, self.xc, self.xt, obs_s, obs_e, lap_off, self.n_obs, ws=self.ws, models=self.models)
        self._advance(self.ws.U, 2 * self.N)
        self.u = self.ws.U[:, 0, :]
        self.t += self.timestep


def ilqr_races(track_table, lap_length, A, B, xcurv0, xglob0, car_s0, car_v, car_ey, steps, vt=0.8, eyt=0.0, N=50, max_iter=150,
               timestep=0.1, device=None, log_every=1, models=None, plant_params=None):
    """xcurv0, xglob0 [B,6]; car_s0, car_v, car_ey [B]: one scripted car per race; models = (A [B,6,6], B [B,6,2]): one model per
    race (host arrays or device tensors); plant_params [B,10]: one car per race.  Returns host arrays: xcurv [T+1,B,6] (T = steps / log_every), u [T,B,2], status [T,B],
    iters [T,B], laps [B]."""
    r = IlqrRaces(track_table, lap_length, A, B, xcurv0, xglob0, car_s0, car_v, car_ey, vt=vt, eyt=eyt, N=N, max_iter=max_iter,
                  timestep=timestep, device=device, models=models, plant_params=plant_params)
    logs = _run_and_log(r.step, steps, log_every,
                        dict(xcurv=lambda: r.xc, u=lambda: r.u, status=lambda: r.ws.status, iters=lambda: r.ws.iters))
    return dict(logs, laps=r.laps.cpu().numpy())


class LmpcLaps(_Plant):
    """B learning-MPC laps at once, device-resident (SURVEY.md section 8f rows 1 + 4): the lap of the reference's racing
    game in which LMPCRacingGame drives alone (tests/auto_racing_game_test.py:60-66 -> utils/base.py:468-517), with the
    race index as the batch dimension.  Per control step and without touching the host:

        crx_lmpc_prep_dev      N stage models from the two previous laps + safe-set selection   (estimate_ABC, control.lmpc :625-639)
        crx_lmpc_solve_dev     the learning-MPC QP                                               (control.lmpc :640-730)
        crx_game_commit_dev    the applied input, u_old and the step counter of add_point
        crx_lmpc_addpoint_dev  the applied (x, u) extends the previous lap's safe set            (add_point)
        crx_plant_step_wrap_dev  plant + lap bookkeeping                                         (forward_dynamics, update_memory)
        crx_game_log_dev       the new state and the applied input join the race's lap log       (update_memory)
        crx_lmpc_addtraj_dev   a race that crossed the line: its logged lap becomes a safe-set lap (add_trajectory)

    Seven libcrx launches per step, in this order; torch only owns the memory.  _plan() is the first two and _apply() is
    add_point + plant: GameLaps builds its step from the same two, so the learning-MPC step is written once.
    Every race carries its own safe set (ss_xcurv [B, L, P, 6], u_ss [B, L, P, 2], qfun [B, L, P], time_ss [B, L]: the
    reference's arrays stored lap-major) and runs lap after lap: the lap hand-over (the reference's test script calls
    add_trajectory between laps, tests/auto_racing_game_test.py) happens per race on the device, until the race's L laps
    of safe-set storage are full (it then keeps racing on its last two laps)."""

    def __init__(self, track_table, lap_length, track_width, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input,
                 N=12, timestep=0.1, device=None, noise_seed=None, plant_params=None, tracks=None, track_id=None):
        _one_track_only("LmpcLaps", tracks, track_id)
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ss, self.us, self.qf = (_dev(a, dev, clone=True) for a in (ss_xcurv, u_ss, qfun))
        self.time_ss, self.it = (_dev(a, dev, torch.int32, clone=True) for a in (time_ss, it))
        Bn, L, P, _ = self.ss.shape
        self.N, self.track_width = N, track_width
        self.lin_points, self.lin_input = _dev(lin_points, dev, clone=True), _dev(lin_input, dev, clone=True)
        self.pdesc = abi.lmpcprep_desc(N, P, L, self.tab.shape[0], timestep, lap_length)   # the prep's descriptor; the plant's is self.plant
        self.desc = abi.lmpc_desc(N=N, n_ss_max=self.pdesc.n_ss_per_lap * self.pdesc.n_ss_laps, ey_max=track_width)
        self.pws = torch_api.LmpcPrepWorkspace(self.pdesc, Bn, dev)
        self.ws = torch_api.LmpcWorkspace(self.desc, Bn, dev)
        self.n_ss = torch.full((Bn,), self.desc.n_ss_max, **i32)
        self.u_old = torch.zeros((Bn, 2), **f64)
        self.u_prev = torch.zeros((Bn, 2), **f64)     # u_old of the last QP launch (bench.py re-issues that launch to time it)
        self.step_no = torch.zeros((Bn,), **i32)
        self.k = 0                     # steps taken by step(); a GameLaps driving this object leaves it at 0
        self._dispatch_of = self       # the object whose `dispatch` orders the QP launch (_order): GameLaps puts itself here
        # the running lap as the simulator logs it (update_memory): states incl. the crossing one, inputs
        self.log_x = torch.zeros((Bn, P, 6), **f64)
        self.log_u = torch.zeros((Bn, P, 2), **f64)
        self.log_x[:, 0] = self.xc
        self.n_log = torch.ones((Bn,), **i32)
        self.laps_prev = torch.zeros((Bn,), **i32)
        self.traj_status = torch.zeros((Bn,), **i32)
        self._ar = torch.arange(Bn, device=dev)
        self._P = P
        self.u = torch.zeros((Bn, 2), **f64)              # the input applied in the last step
        self.addpoint_step = torch.zeros((Bn,), **i32)
        self.crossed = torch.zeros((Bn,), **i32)

    def log_and_handover(self, u):
        """After the plant step: append (new state, applied input) to every race's lap log -- the crossing state with its s
        unwrapped, like update_memory -- (crx_game_log_dev) and hand the completed laps over to the safe set
        (crx_lmpc_addtraj_dev)."""
        torch_api.game_log_dev(self.lap_length, self.xc, u, self.laps, self.laps_prev, self.log_x, self.log_u, self.n_log, self.crossed)
        torch_api.lmpc_addtraj_dev(self.pdesc, self.crossed, self.log_x, self.log_u, self.n_log, self.ss, self.us, self.qf, self.time_ss, self.it,
                                   self.step_no, self.xc, self.traj_status)

    def log_and_handover_torch(self, u):
        """log_and_handover written as element-wise torch ops (round 2; kept as an independent restatement for the tests)."""
        crossed = (self.laps > self.laps_prev).to(torch.int32)
        self.laps_prev.copy_(self.laps)
        xu = self.xc.clone()
        xu[:, 4] += self.lap_length * crossed.to(torch.float64)       # (an int32 tensor times a Python float would be float32)
        n = self.n_log.long()
        self.log_x[self._ar, torch.clamp(n, max=self._P - 1)] = xu
        self.log_u[self._ar, torch.clamp(n - 1, min=0, max=self._P - 1)] = u
        self.n_log += 1
        torch_api.lmpc_addtraj_dev(self.pdesc, crossed, self.log_x, self.log_u, self.n_log, self.ss, self.us, self.qf, self.time_ss, self.it,
                                   self.step_no, self.xc, self.traj_status)

    def _plan(self, lin_points, lin_input, from_plan, active=None):
        """The stage models and safe-set points around (lin_points, lin_input) -- from_plan: a previous plan, shifted by one stage
        inside the kernel (control.py:726-728) -- and the learning-MPC QP on them: lmpc_prep_dev, lmpc_solve_dev, with one
        longest_first between them under that dispatch.  active: int32 mask [B] for both launches."""
        torch_api.lmpc_prep_dev(self.pdesc, self.ss, self.us, self.qf, self.time_ss, self.it, self.xc, lin_points, lin_input, self.tab,
                                from_plan, ws=self.pws, active=active)
        torch_api.lmpc_solve_dev(self.desc, self.xc, self.u_old, self.pws.A, self.pws.B, self.pws.C, self.pws.ss, self.pws.qfun, self.n_ss,
                                 ws=self.ws, active=active, order=_order(self._dispatch_of, self.ws.iters, active))

    def _apply(self, u, u_stride, addpoint_step):
        """The applied (x, u) joins the safe set at addpoint_step [B] (negative: not for this race) and the plant moves:
        lmpc_addpoint_dev, plant_step_wrap_dev."""
        torch_api.lmpc_addpoint_dev(self.pdesc, self.ss, self.us, self.time_ss, self.it, addpoint_step, self.xc, u, u_stride)
        self._advance(u, u_stride)

    def step(self, torch_glue=False):
        """One control step of every race, seven libcrx launches: lmpc_prep_dev, lmpc_solve_dev, game_commit_dev, lmpc_addpoint_dev,
        plant_step_wrap_dev, game_log_dev, lmpc_addtraj_dev (the lap hand-over).
        torch_glue = True: the bookkeeping as element-wise torch ops instead of crx_game_commit_dev / crx_game_log_dev (round 2's
        formulation, kept for the tests: both must produce the same bits), which leaves five."""
        N = self.N
        if self.k == 0:     # first call of the lap: linearisation points handed over by the previous controller (utils/base.py:651-653)
            self._plan(self.lin_points, self.lin_input, False)
        else:               # afterwards: the previous plan
            self._plan(self.ws.X, self.ws.U, True)
        if torch_glue:
            self._apply(self.ws.U, 2 * N, self.step_no)
            self.u_prev.copy_(self.u_old)
            self.u_old.copy_(self.ws.U[:, 0, :])
            self.u.copy_(self.u_old)
            self.step_no += 1
            self.k += 1
            self.log_and_handover_torch(self.u_old)
            return
        # applied input, plan hand-over (u_old; lin_points / lin_input are the shifted plan), step counter: one launch
        torch_api.game_commit_dev(N, N, None, None, self.ws.X, self.ws.U, None, self.u, self.u_old, self.u_prev, self.lin_points, self.lin_input,
                                  self.step_no, self.addpoint_step, None)
        self._apply(self.u, 2, self.addpoint_step)
        self.k += 1
        self.log_and_handover(self.u)


def lmpc_laps(track_table, lap_length, track_width, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input, steps,
              N=12, timestep=0.1, device=None, noise_seed=None, plant_params=None):
    """Run `steps` control steps of B learning-MPC laps (plant_params [B,10]: one car per lap); returns host logs xcurv [steps+1, B, 6], u [steps, B, 2], status [steps, B]
    (QP status), prep_status [steps, B] (singular regression: the stage keeps its previous / zero model rows), laps [B],
    traj_status [B] (lap hand-over: 1 = safe-set storage full)."""
    r = LmpcLaps(track_table, lap_length, track_width, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input, N=N,
                 timestep=timestep, device=device, noise_seed=noise_seed, plant_params=plant_params)
    logs = _run_and_log(r.step, steps, 1, dict(xcurv=lambda: r.xc, u=lambda: r.u_old, status=lambda: r.ws.status,
                                               prep_status=lambda: r.pws.status))
    return dict(logs, laps=r.laps.cpu().numpy(),
                traj_status=r.traj_status.cpu().numpy())   # 1: the race's n_laps of safe-set storage were full at its last hand-over


class GameLaps:
    """B laps of the racing game WITH traffic at once, device-resident (the row's stated purpose:
    the closed-loop Monte-Carlo of the overtaking game, car_racing/tests/overtake_planner_test.py:307-309): per control step,
    LMPCRacingGame.calc_input (utils/base.py:456-583) for every race --

        scripted cars' states and predictions (NoDynamicsModel, utils/base.py:847-890; element-wise torch ops)
        crx_planner_scene_dev      vehicles of interest, partial sort, veh_infos                 (get_overtake_flag, get_local_traj :64-92)
      overtake branch (:518-582)
        crx_planner_prep_dev       Bezier references, ey bounds                                   (:94-117, 277-324)
        crx_planner_plan_dev       the region QPs + selection                                     (solve_optimization_problem)
        crx_track_prep_dev         per-stage targets, obstacle window / packing                   (control.mpc_multi_agents :293-382)
        crx_cbf_solve_dev          the tracking NLP with CBF rows                                 (:270-473)
      learning-MPC branch (:468-517)
        crx_lmpc_prep_dev, crx_lmpc_solve_dev, crx_lmpc_addpoint_dev
      crx_plant_step_wrap_dev

    Every launch covers the whole batch; the heavy kernels of a branch (tracking NLP; regression + learning-MPC QP) are
    MASKED launches (crx_*_masked_dev): the wavefront of a race that is in the other branch returns at once -- the region
    QPs of the planner included; the cheap kernels around them (scene, prep, selection, tracking prep) run for every race.  The applied input, the
    plan hand-over (u_old, linearisation points), add_point and the direction flag are taken from the branch the race is
    in; no host round trip, no compaction.  Fourteen libcrx launches per step (thirteen with planner = "path"), listed at step();
    the learning-MPC ones are LmpcLaps._plan / _apply / log_and_handover of `lm`, which also holds the plant (lm.xc, lm.xc_next, ...).

    planner = "path" (LMPCRacingGame(path_planner=True), planning/overtake_path_planner.py): the overtake branch becomes
        crx_path_plan_dev          obstacle rows, control points, samples, side rows; the region QPs; arg-min + target (include/crx.h P1-P8)
        crx_track_prep_dev         on the path planner's target trajectory
        crx_cbf_solve_dev          the tracking NLP
    with the scene, the masks, the commit (which takes the path planner's flag) and the learning-MPC branch as they are.  alpha =
    racing_game_param.alpha, the weight of the Bezier reference in the path QPs.  models = only the tracking NLP has dynamics here.
    planner = "traj" (default) is the loop above, call for call.  plant_params [B,10]: one car per race, handed to `lm`, which holds the plant."""

    def __init__(self, track_table, lap_length, track_width, A, B, opt_xcurv, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0,
                 lin_points, lin_input, car_s0, car_v, car_ey, N=12, N_plan=10, timestep=0.1, device=None, noise_seed=None, models=None,
                 planner="traj", alpha=0.98, plant_params=None, tracks=None, track_id=None):
        _one_track_only(type(self).__name__, tracks, track_id)
        if planner not in ("traj", "path"):
            raise ValueError("planner must be 'traj' or 'path', got %r" % (planner,))
        self.planner = planner
        self.lm = LmpcLaps(track_table, lap_length, track_width, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input,
                           N=N, timestep=timestep, device=device, noise_seed=noise_seed, plant_params=plant_params)
        lm = self.lm
        lm._dispatch_of = self         # bench.py sets `dispatch` on the game
        dev = lm.device
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        Bn = lm.batch
        self.s0, self.v, self.ey = (_dev(a, dev) for a in (car_s0, car_v, car_ey))
        VA = self.s0.shape[1]
        V = min(VA, abi.CRX_MAX_VEH)
        self.Np, self.V, self.VA, self.L = N_plan, V, VA, lap_length
        self.track_width = track_width
        if models is not None and A is None and B is None:   # (the descriptors' own model is not read then)
            A, B = np.zeros((6, 6)), np.zeros((6, 2))
        self.scene = abi.scene_desc(N_plan, VA, V, lap_length)
        self.prep = abi.prep_desc(N_plan, V, opt_xcurv.shape[0], track_width, lap_length)
        self.plan, self.sel = abi.planner_desc(N_plan, A, B), abi.select_desc(N_plan, V, lap_length)
        self.track_desc = abi.cbf_desc(N_plan, V, A, B, Q=(10.0, 0, 0, 5.0, 0, 50.0), R=(0.1, 0.1), alpha=0.6, margin=0.15,
                                       ey_max=track_width, per_stage_target=True, l_sum=0.4, w_sum=0.2)
        self.opt_s, self.opt_ey = _dev(opt_xcurv[:, 4], dev), _dev(opt_xcurv[:, 5], dev)
        self.sws = torch_api.SceneWorkspace(self.scene, Bn, dev)
        self.pws = torch_api.PrepWorkspace(self.prep, Bn, dev)
        self.qws = torch_api.PlannerWorkspace(self.plan, Bn * (V + 1), dev)
        self.selws = torch_api.SelectWorkspace(self.sel, Bn, dev)
        self.tws = torch_api.CbfWorkspace(self.track_desc, Bn, dev)
        self.flag = self.selws.flag    # the direction flag the commit takes: the trajectory planner's selection, or the path planner's
        if planner == "path":          # LMPCRacingGame(path_planner=True): alpha = racing_game_param.alpha (utils/base.py:379-408)
            self.pathprep = abi.pathprep_desc(N_plan, V, VA, opt_xcurv.shape[0], track_width, lap_length)
            self.pathqp = abi.path_desc(N_plan, alpha)
            self.opt_vx = _dev(opt_xcurv[:, 0], dev)
            self.ppws = torch_api.PathPlanWorkspace(self.pathprep, Bn, dev)
            self.ppws.target.zero_()   # (a race that has never planned: its rows are read by the tracking prep, whose NLP is masked out)
            self.flag = self.ppws.flag
        # models = (A [B,6,6], B [B,6,2]), host arrays or device tensors (PidLaps.identify(): held, not copied): the overtake branch of race b
        # on ITS model -- its V + 1 region QPs (crx_planner_plan_models_dev) and its tracking NLP (crx_cbf_solve_models_dev); A, B above are
        # then unused.  Both reach tables are computed here, once.  The learning-MPC branch identifies its own stage models, as before.
        # planner="path": only the tracking NLP has dynamics (the path QPs are geometric)
        self.plan_models = self.track_models = None
        if models is not None:
            mA, mB = _models(models[0], models[1], Bn, dev)
            if planner == "traj":
                self.plan_models = torch_api.PlannerModels(self.plan, mA, mB, regions=V + 1)
            self.track_models = torch_api.CbfModels(self.track_desc, mA, mB)
        self.xt = torch.empty((Bn, N_plan + 1, 6), **f64)
        self.obs_s, self.obs_e = torch.empty((Bn, V, N_plan + 1), **f64), torch.empty((Bn, V, N_plan + 1), **f64)
        self.lap_off, self.n_obs = torch.empty((Bn, V), **f64), torch.empty((Bn,), **i32)
        self.n_all = torch.full((Bn,), VA, **i32)
        self.old_flag = torch.full((Bn,), -1, **i32)
        self.jdt = torch.arange(N_plan + 1, **f64) * timestep
        self.veh = torch.zeros((Bn, VA, 6), **f64)
        self.u = torch.zeros((Bn, 2), **f64)
        self.lin_points, self.lin_input = lm.lin_points.clone(), lm.lin_input.clone()
        self.neg = torch.full((Bn,), -(1 << 20), **i32)
        self.overtake = torch.zeros((Bn,), dtype=torch.bool, device=dev)
        self.m_ot, self.m_lm = torch.zeros((Bn,), **i32), torch.zeros((Bn,), **i32)
        self.pred_s, self.pred_e = torch.zeros((Bn, VA, N_plan + 1), **f64), torch.zeros((Bn, VA, N_plan + 1), **f64)
        self.overflow_seen = torch.zeros((Bn,), **i32)    # scene overflow (more vehicles of interest than slots), accumulated
        # the two branches of a step are independent until the commit: their kernels go to two HIP streams and overlap (the
        # masked launches of a branch leave part of the chip idle: a third of the races plan and track, the rest regress and solve)
        self.s_ot = self.s_lm = None   # set_branch_streams, or two of libcrx's at the first step
        self.overlap = True            # False: both branches on the caller's stream, one after the other
        self.t = 0.0

    def step(self):
        """One control step of every race, fourteen libcrx launches: game_traffic_dev (_traffic()), planner_scene_dev, game_masks_dev; the
        overtake branch planner_prep_dev, planner_plan_dev (planner = "path": path_plan_dev for the two), track_prep_dev,
        cbf_solve_dev; the learning-MPC branch lmpc_prep_dev, lmpc_solve_dev; game_commit_dev, lmpc_addpoint_dev,
        plant_step_wrap_dev, game_log_dev, lmpc_addtraj_dev (the lap hand-over).  lm.k stays 0: the game plans from its own
        linearisation points, which the commit keeps."""
        lm, L, N = self.lm, self.L, self.lm.N
        self._traffic()
        torch_api.planner_scene_dev(self.scene, lm.xc, self.n_all, self.veh, self.pred_s, self.pred_e, ws=self.sws)
        torch_api.game_masks_dev(self.sws.n_veh, self.m_ot, self.m_lm, overflow=self.sws.overflow, overflow_seen=self.overflow_seen)
        self.overtake = self.m_ot                                  # int32 mask; bool(overtake[b]) = race b is in the overtake branch
        self._branches(self.m_ot, self.m_lm, overlap=self.overlap)
        torch_api.game_commit_dev(N, self.Np, self.m_ot, self.tws.U, lm.ws.X, lm.ws.U, self.flag, self.u, lm.u_old, lm.u_prev,
                                  self.lin_points, self.lin_input, lm.step_no, lm.addpoint_step, self.old_flag)
        lm._apply(self.u, 2, lm.addpoint_step)
        self.t += lm.timestep
        lm.log_and_handover(self.u)

    def _traffic(self):
        """The step's first launch: the other vehicles' states veh and predictions pred_s, pred_e [B,VA,..] that the scene reads with n_all --
        here the scripted cars at the game's clock (game_traffic_dev).  FieldGames puts the other driven cars of the race there."""
        torch_api.game_traffic_dev(self.Np, self.L, self.t, self.lm.timestep, self.s0, self.v, self.ey, self.veh, self.pred_s, self.pred_e)

    def stats_inputs(self):
        """As _Plant.stats_inputs, answered from `lm` (which holds the plant): the scripted cars at the game's clock, and the branch
        mask of the last step as the flag (RaceStats counts the samples a race spent in the overtake branch)."""
        return self.lm.stats_inputs(t=self.t, car_s0=self.s0, car_v=self.v, car_ey=self.ey, flag=self.m_ot)

    def set_branch_streams(self, s_ot, s_lm):
        """The two streams the branches of a step run on (crx.montecarlo.Concurrent hands out streams it measured to overlap)."""
        self.s_ot, self.s_lm = s_ot, s_lm

    def _branches(self, m_ot, m_lm, overlap=False):
        """The solver launches of both branches (masked: every race runs its own branch's kernels only); overlap: each branch
        on its own stream, forked from and joined to the current one."""
        if overlap and self.s_ot is None:
            (self.s_ot, self.s_lm), nc = torch_api.new_streams(2, self.lm.xc.device)
            if nc < 2:
                overlap = self.overlap = False
        if overlap:
            cur = torch.cuda.current_stream(self.lm.xc.device)
            self.s_ot.wait_stream(cur); self.s_lm.wait_stream(cur)
            with torch.cuda.stream(self.s_ot):
                self._branch_overtake(m_ot)
            with torch.cuda.stream(self.s_lm):
                self._branch_lmpc(m_lm)
            cur.wait_stream(self.s_ot); cur.wait_stream(self.s_lm)
        else:
            self._branch_overtake(m_ot)
            self._branch_lmpc(m_lm)

    def _branch_overtake(self, m_ot):
        """The scene's planner produces the target trajectory; the tracking prep and the tracking NLP on it are the same for both."""
        xc, sw = self.lm.xc, self.sws
        if self.planner == "path":   # one launch: prep, region QPs, selection + target
            torch_api.path_plan_dev(self.pathprep, self.pathqp, xc, xc, sw.n_veh, sw.order, self.veh, sw.max_dv, sw.obs_ey, self.opt_s,
                                    self.opt_ey, self.opt_vx, ws=self.ppws, active=m_ot)
            target = self.ppws.target
        else:
            torch_api.planner_prep_dev(self.prep, xc, xc, sw.n_veh, sw.veh_info, sw.max_dv, sw.obs_s, sw.obs_ey, self.opt_s, self.opt_ey,
                                       ws=self.pws)
            torch_api.planner_plan_dev(self.plan, self.sel, self.pws.x0, self.pws.bez_s, self.pws.bez_ey, self.pws.ey_lb, self.pws.ey_ub,
                                       sw.n_veh, sw.obs_s, sw.obs_ey, self.old_flag, self.qws, self.selws, active=m_ot, models=self.plan_models)
            target = self.selws.best_X
        torch_api.track_prep_dev(self.Np, self.V, self.L, xc, sw.n_veh, sw.obs_s, sw.obs_ey, target, self.xt, self.obs_s, self.obs_e,
                                 self.lap_off, self.n_obs)
        torch_api.cbf_solve_dev(self.track_desc, xc, self.xt, self.obs_s, self.obs_e, self.lap_off, self.n_obs, ws=self.tws, active=m_ot,
                                order=_order(self, self.tws.iters, m_ot), models=self.track_models)

    def _branch_lmpc(self, m_lm):
        self.lm._plan(self.lin_points, self.lin_input, False, active=m_lm)

    def step_torch(self):
        """The same control step with the bookkeeping written as element-wise torch ops (round 2's formulation, ~40 small launches;
        kept as an independent restatement for the tests: step() must produce the same bits)."""
        lm, L, N = self.lm, self.L, self.lm.N
        # scripted cars at their own clock t: s = v t + s0 (wrapped once past the line, update_memory), predictions unwrapped (quirk Q6)
        s_now = self.v * self.t + self.s0
        self.veh[:, :, 0] = self.v
        self.veh[:, :, 4] = s_now - L * torch.clamp(torch.ceil(s_now / L) - 1.0, min=0.0)   # update_memory: wrapped whenever s > L, lap after lap
        self.veh[:, :, 5] = self.ey
        pred_s = (self.v[:, :, None] * (self.t + self.jdt)[None, None, :] + self.s0[:, :, None]).contiguous()
        pred_e = (self.ey[:, :, None] + 0.0 * self.jdt[None, None, :]).contiguous()
        torch_api.planner_scene_dev(self.scene, lm.xc, self.n_all, self.veh, pred_s, pred_e, ws=self.sws)
        self.overtake = self.sws.n_veh > 0
        m_ot = self.overtake.to(torch.int32)                      # masked launches: every race runs its own branch's kernels only
        m_lm = 1 - m_ot
        self._branches(m_ot, m_lm)
        # ---- the branch each race is in
        ot = self.overtake
        self.u.copy_(torch.where(ot[:, None], self.tws.U[:, 0, :], lm.ws.U[:, 0, :]))
        addpoint_step = torch.where(ot, self.neg, lm.step_no)     # add_point's step: the counter before it advances below
        lm.u_prev.copy_(lm.u_old)
        lm.u_old.copy_(torch.where(ot[:, None], lm.u_old, lm.ws.U[:, 0, :]))
        X, U = lm.ws.X, lm.ws.U
        self.lin_points.copy_(torch.where(ot[:, None, None], self.lin_points, torch.cat((X[:, 1:], X[:, -1:]), dim=1)))
        self.lin_input.copy_(torch.where(ot[:, None, None], self.lin_input, torch.cat((U[:, 1:], U[:, -1:]), dim=1)))
        lm.step_no += (~ot).to(torch.int32)
        self.old_flag.copy_(torch.where(ot, self.flag, torch.full_like(self.old_flag, -1)))
        lm._apply(self.u, 2, addpoint_step)
        self.t += lm.timestep
        lm.log_and_handover_torch(self.u)


def game_laps(track_table, lap_length, track_width, A, B, opt_xcurv, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input,
              car_s0, car_v, car_ey, steps, device=None, noise_seed=None, models=None, planner="traj", alpha=0.98, plant_params=None):
    """Run `steps` control steps of B racing-game laps with scripted traffic; models = (A [B,6,6], B [B,6,2]): the overtake branch of
    every race (region QPs, tracking NLP) on its own model.  planner = "path": the overtake path planner (GameLaps) in that branch.  Host logs: xcurv [steps+1, B, 6], u [steps, B, 2],
    overtake [steps, B] (which branch), flag [steps, B] (direction flag, -1 in the LMPC branch), cars_s [steps, B, V], laps [B]."""
    r = GameLaps(track_table, lap_length, track_width, A, B, opt_xcurv, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points, lin_input,
                 car_s0, car_v, car_ey, device=device, noise_seed=noise_seed, models=models, planner=planner, alpha=alpha,
                 plant_params=plant_params)
    logs = _run_and_log(r.step, steps, 1, dict(xcurv=lambda: r.lm.xc, u=lambda: r.u, overtake=lambda: r.overtake.bool(),
                                               flag=lambda: r.old_flag, cars_s=lambda: r.v * r.t + r.s0),
                        before=("cars_s",))    # where the scripted cars are when the step plans
    return dict(logs, laps=r.lm.laps.cpu().numpy(), traj_status=r.lm.traj_status.cpu().numpy(),
                scene_overflow=r.overflow_seen.cpu().numpy())


class FieldGames(GameLaps):
    """R races of C cars that ALL play the racing game: every car is the ego of its own LMPCRacingGame.calc_input -- its own safe set, its
    own learning MPC, its own overtake planner and tracking NLP -- and a vehicle of the C - 1 others, which it sees as the reference's
    planner sees a driven opponent: the current state and the zero-input roll-out get_trajectory_nsteps(N + 1)
    (planning/overtake_traj_planner.py:77-85, racing/offboard.py:51-94).  The loop is GameLaps with batch R*C (race-major, car-minor) whose
    first launch is crx_field_traffic_dev (include/crx.h "Field games", F1-F3, F6, G1-G3) where GameLaps has crx_game_traffic_dev; every
    launch after it is GameLaps', call for call.  All cars of a step see the states at the start of the step (F1).

    The per-car learning-MPC inputs [R*C, ...] are those of LmpcLaps / GameLaps, host arrays or device tensors.  A learning-MPC lap begins
    at the line and every seeded car stands there, so a field is built from grid_start(SeedLaps.lmpc_inputs(), k, track), which also
    returns step_no, n_log, log_x, log_u, u_old, u_prev: the bookkeeping of a car that is k steps into its lap; they are applied to `lm`
    after it is built (None: the lap has just begun, as LmpcLaps starts).  FieldGames(..., n_cars, **grid_start(...)) takes them all.
    models = (A [R*C,6,6], B [R*C,6,2]), plant_params [R*C,10], planner = "traj" | "path": as GameLaps."""

    def __init__(self, track_table, lap_length, track_width, A, B, opt_xcurv, n_cars, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0,
                 lin_points, lin_input, step_no=None, n_log=None, log_x=None, log_u=None, u_old=None, u_prev=None, N=12, N_plan=10,
                 timestep=0.1, device=None, noise_seed=None, models=None, planner="traj", alpha=0.98, plant_params=None, tracks=None,
                 track_id=None):
        _one_track_only("FieldGames", tracks, track_id)
        Cn = int(n_cars)
        if not 1 <= Cn <= abi.CRX_MAX_VEH + 1:
            raise ValueError("1 .. %d cars per race" % (abi.CRX_MAX_VEH + 1))
        Bn = int(xcurv0.shape[0])
        if Bn % Cn:
            raise ValueError("xcurv0: %d cars do not make races of %d" % (Bn, Cn))
        none = np.zeros((Bn, max(Cn - 1, 1)))      # no scripted car: the slots of the scene are the other cars of the race (one idle slot with C = 1)
        super().__init__(track_table, lap_length, track_width, A, B, opt_xcurv, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points,
                         lin_input, none, none, none, N=N, N_plan=N_plan, timestep=timestep, device=device, noise_seed=noise_seed, models=models,
                         planner=planner, alpha=alpha, plant_params=plant_params)
        del self.s0, self.v, self.ey
        lm = self.lm
        self.n_cars, self.n_races = Cn, Bn // Cn
        self.fdesc = abi.field_desc(N_plan, Cn, lm.tab.shape[0], lap_length, dt=timestep)
        self.fws = torch_api.FieldTrafficWorkspace(self.fdesc, self.n_races, lm.device)
        # what the scene and the path planner read of the other vehicles is what the traffic launch writes
        self.veh, self.pred_s, self.pred_e, self.n_all = self.fws.veh_xcurv, self.fws.pred_s, self.fws.pred_ey, self.fws.n_all
        # the grid fields: a car that is k steps into its lap (grid_start)
        for dst, src, dtype in ((lm.step_no, step_no, torch.int32), (lm.n_log, n_log, torch.int32), (lm.log_x, log_x, torch.float64),
                                (lm.log_u, log_u, torch.float64), (lm.u_old, u_old, torch.float64), (lm.u_prev, u_prev, torch.float64)):
            if src is not None:
                dst.copy_(_dev(src, lm.device, dtype).reshape(dst.shape))

    def _traffic(self):
        """field_traffic_dev: every car's roll-out, and per ego the other cars of its race as the scene's vehicles."""
        torch_api.field_traffic_dev(self.fdesc, self.lm.tab, self.lm.xc, self.fws)

    def stats_inputs(self):
        """The field form: the opponents of a car are the other cars of its race, CarParam's dimensions for every pair, and the branch
        mask of the last step as the flag."""
        return self.lm.stats_inputs(n_cars=self.n_cars, l_sum=0.4, w_sum=0.2, flag=self.m_ot)


def field_games(track_table, lap_length, track_width, A, B, opt_xcurv, n_cars, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points,
                lin_input, steps, device=None, noise_seed=None, models=None, planner="traj", alpha=0.98, plant_params=None, **grid):
    """Run `steps` control steps of R races of n_cars cars that all play the racing game (FieldGames; **grid: the grid fields of
    grid_start).  Host logs: xcurv [steps+1, R*C, 6], u [steps, R*C, 2], overtake [steps, R*C] (which branch), flag [steps, R*C] (direction
    flag, -1 in the LMPC branch), laps [R*C], traj_status [R*C]."""
    r = FieldGames(track_table, lap_length, track_width, A, B, opt_xcurv, n_cars, ss_xcurv, u_ss, qfun, time_ss, it, xcurv0, xglob0, lin_points,
                   lin_input, device=device, noise_seed=noise_seed, models=models, planner=planner, alpha=alpha, plant_params=plant_params, **grid)
    logs = _run_and_log(r.step, steps, 1, dict(xcurv=lambda: r.lm.xc, u=lambda: r.u, overtake=lambda: r.overtake.bool(),
                                               flag=lambda: r.old_flag))
    return dict(logs, laps=r.lm.laps.cpu().numpy(), traj_status=r.lm.traj_status.cpu().numpy())


def grid_start(inputs, k, track):
    """Several learning-MPC cars on one track.  A learning-MPC lap must begin at the line (the lap log, add_point's row index, time_ss and
    Qfun all count from the crossing) and every seeded car stands there; grid_start puts car b where it was k[b] steps into its OWN last
    safe-set lap, j = it[b] - 1, with every piece of per-car bookkeeping as if it had just driven those k[b] steps again and reproduced
    that lap: the arrays equal, bit for bit, what game_commit_dev (with the plan X[m] = ss[b,j,i+m], U[m] = us[b,j,i+m] at step i),
    lmpc_addpoint_dev and game_log_dev (with the new state ss[b,j,i+1]) leave behind after k[b] steps from ss[b,j,0]
    (tests/test_gpu_field_game.py replays them).  Cars of a race get different k and so stand apart.

    inputs: the dict of SeedLaps.lmpc_inputs(), tensors or host arrays; k [B] integers, 0 <= k[b] <= time_ss[b,j] - N - 1; track: the
    mirror's ClosedTrack (lap_length, get_global_position, get_orientation).  Set-up work, torch index operations on the inputs' device and
    one host pass for the global poses; no kernel.  Returns the inputs' names plus step_no, n_log, log_x, log_u, u_old, u_prev -- the
    arguments of FieldGames.  For car b with k = k[b] > 0 (a car with k = 0 keeps every input and the fields of a lap just begun):
        xcurv0 = ss[b,j,k];  xglob0: velocities copied, pose from the track at (s, ey, epsi)
        lin_points[m] = ss[b,j,k-1+min(m+1,N)], lin_input[m] = us[b,j,k-1+min(m+1,N-1)]   (the plan shifted by a stage, its last one repeated)
        step_no = k, n_log = k + 1, log_x[:k+1] = ss[b,j,:k+1], log_u[:k] = us[b,j,:k], u_old = us[b,j,k-1], u_prev = us[b,j,k-2] (zero for k = 1)
        for i < k, row time_ss[b,j] + i + 1 of lap j (while below n_points): ss[b,j,i] + (0,0,0,0,L,0) and us[b,j,i]   (add_point)"""
    t = {name: (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))) for name, a in inputs.items()}
    ss, us = t["ss_xcurv"].to(torch.float64), t["u_ss"].to(torch.float64)
    dev = ss.device
    Bn, _, P, _ = ss.shape
    N = t["lin_input"].shape[1]
    ar = torch.arange(Bn, device=dev)
    k = torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k), dtype=torch.int64, device=dev).reshape(-1)
    j = t["it"].to(torch.int64) - 1
    if k.shape[0] != Bn or bool((j < 0).any()) or bool((j >= ss.shape[1]).any()):
        raise ValueError("grid_start: one k per car and at least one safe-set lap per car (it >= 1)")
    T = t["time_ss"].to(torch.int64)[ar, j]
    if bool(((k < 0) | (k > T - N - 1)).any()):
        raise ValueError("grid_start: 0 <= k[b] <= time_ss[b, it[b]-1] - N - 1 = %s, got %s" % ((T - N - 1).tolist(), k.tolist()))
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    xcurv0 = t["xcurv0"].to(torch.float64)
    log_x, log_u = torch.zeros((Bn, P, 6), **f64), torch.zeros((Bn, P, 2), **f64)
    log_x[:, 0] = xcurv0
    out = dict(t, step_no=torch.zeros(Bn, **i32), n_log=torch.ones(Bn, **i32), log_x=log_x, log_u=log_u, u_old=torch.zeros((Bn, 2), **f64),
               u_prev=torch.zeros((Bn, 2), **f64))
    moved = k > 0
    if not bool(moved.any()):
        return out
    lapx, lapu = ss[ar, j], us[ar, j]                                      # [B,P,6], [B,P,2]: every car's lap j
    m1, m2 = moved[:, None], moved[:, None, None]
    out["xcurv0"] = torch.where(m1, lapx[ar, k], xcurv0)
    rows_x = (k - 1)[:, None] + torch.clamp(torch.arange(N + 1, device=dev) + 1, max=N)[None, :]
    rows_u = (k - 1)[:, None] + torch.clamp(torch.arange(N, device=dev) + 1, max=N - 1)[None, :]
    out["lin_points"] = torch.where(m2, lapx[ar[:, None], rows_x.clamp(min=0)], t["lin_points"].to(torch.float64))
    out["lin_input"] = torch.where(m2, lapu[ar[:, None], rows_u.clamp(min=0)], t["lin_input"].to(torch.float64))
    out["step_no"], out["n_log"] = k.to(torch.int32), (k + 1).to(torch.int32)
    row = torch.arange(P, device=dev)[None, :]
    out["log_x"] = torch.where(m2 & (row <= k[:, None])[:, :, None], lapx, log_x)
    out["log_u"] = torch.where((row < k[:, None])[:, :, None], lapu, log_u)
    out["u_old"] = torch.where(k[:, None] >= 1, lapu[ar, (k - 1).clamp(min=0)], out["u_old"])
    out["u_prev"] = torch.where(k[:, None] >= 2, lapu[ar, (k - 2).clamp(min=0)], out["u_prev"])
    # the rows add_point would have written (crx_lmpc_addpoint_dev: row time_ss + step + 1 of lap j, dropped at n_points)
    i = torch.arange(int(k.max()), device=dev)[None, :]
    b_idx, i_idx = torch.nonzero((i < k[:, None]) & (T[:, None] + i + 1 < P), as_tuple=True)
    off = torch.zeros(6, **f64)
    off[4] = float(track.lap_length)
    ss2, us2 = ss.clone(), us.clone()
    ss2[b_idx, j[b_idx], T[b_idx] + i_idx + 1] = lapx[b_idx, i_idx] + off
    us2[b_idx, j[b_idx], T[b_idx] + i_idx + 1] = lapu[b_idx, i_idx]
    out["ss_xcurv"], out["u_ss"] = ss2, us2
    # the global pose that goes with the curvilinear state: the host's one pass
    xc = out["xcurv0"].cpu().numpy()
    xg = np.array(t["xglob0"].cpu().numpy(), dtype=float)
    for b in np.nonzero(moved.cpu().numpy())[0]:
        xg[b, 0:3] = xc[b, 0:3]
        xg[b, 3] = track.get_orientation(xc[b, 4], xc[b, 5]) + xc[b, 3]
        xg[b, 4], xg[b, 5] = track.get_global_position(xc[b, 4], xc[b, 5])
    out["xglob0"] = torch.as_tensor(xg, **f64)
    return out


class PidLaps(_Plant):
    """B copies of the reference's identification experiment (car_racing/tests/system_identification_test.py: one car under
    PIDTracking on its own, logged for `steps` control steps), device-resident, then identified without leaving the device.
    Per control step: ONE crx_plant_step_noise_dev (with the lap wrap of update_memory, base.py:795-819) and ONE crx_pid_log_dev
    that logs the step's row and computes the next input.  x_log [B,T,6] holds xcurv_log (s wrapped, S2) and u_log [B,T,2]
    what get_udata assembles from it (S5: u[k] = the input applied in the step that produced x[k]).
    Noise: noise_z [T,B,3] standard-normal draws (the reference's three randn per step, in call order), else a device generator
    seeded with noise_seed; both None = zero noise.  plant_params [B,10]: every car its own BicycleDynamicsParam set, so that identify()
    returns the models of B different cars."""

    def __init__(self, track_table, lap_length, xcurv0, xglob0, steps, vt=0.5, eyt=0.0, timestep=0.1, noise_z=None,
                 noise_seed=None, device=None, plant_params=None, tracks=None, track_id=None):
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params, tracks, track_id)
        f64 = dict(dtype=torch.float64, device=dev)
        Bn, T = self.batch, int(steps)
        self.steps = T
        self.vt, self.eyt = _per_race(vt, Bn, dev), _per_race(eyt, Bn, dev)
        self.noise_z = None
        if noise_z is not None:
            self.noise_z = noise_z.to(**f64) if torch.is_tensor(noise_z) else _dev(noise_z, dev)
            if tuple(self.noise_z.shape) != (T, Bn, 3):
                raise ValueError("noise_z: expected shape %s, got %s" % ((T, Bn, 3), tuple(self.noise_z.shape)))
        self.x_log = torch.zeros((Bn, T, 6), **f64)
        self.u_log = torch.zeros((Bn, T, 2), **f64)
        self.u, self.u_next = torch.zeros((Bn, 2), **f64), torch.zeros((Bn, 2), **f64)
        self.k = 0
        torch_api.pid_log_dev(T, -1, self.vt, self.eyt, self.xc, None, self.u, self.x_log, self.u_log)

    def step(self):
        """One control step of every car: plant_step_wrap_dev, pid_log_dev."""
        k = self.k
        self._advance(self.u, 2, noise_z=None if self.noise_z is None else self.noise_z[k])
        torch_api.pid_log_dev(self.steps, k, self.vt, self.eyt, self.xc, self.u, self.u_next if k + 1 < self.steps else None,
                              self.x_log, self.u_log)
        self.u, self.u_next = self.u_next, self.u
        self.k += 1

    def run(self):
        while self.k < self.steps:
            self.step()
        return self

    def identify(self, lamb=1e-9, group_offsets=None, chunk_rows=8192):
        """crx_sysid_fit_dev over the resident logs: one fit per car (group_offsets None) or per group of cars."""
        T, Bn = self.steps, self.batch
        offsets = torch.arange(Bn + 1, dtype=torch.int64, device=self.device) * T
        return torch_api.sysid_fit_dev(abi.sysid_desc(lamb, chunk_rows=chunk_rows), self.x_log.view(-1, 6), self.u_log.view(-1, 2),
                                       offsets, group_offsets, max_log_rows=T)


def pid_laps(track_table, lap_length, xcurv0, xglob0, steps, vt=0.5, eyt=0.0, timestep=0.1, noise_z=None, noise_seed=None,
             device=None, plant_params=None, tracks=None, track_id=None):
    """PidLaps run to the end: the logs stay on the device (r.x_log, r.u_log); r.identify(lamb) fits them.  tracks (abi.track_set),
    track_id [B]: car b on its own track (track_table and lap_length None)."""
    return PidLaps(track_table, lap_length, xcurv0, xglob0, steps, vt=vt, eyt=eyt, timestep=timestep, noise_z=noise_z,
                   noise_seed=noise_seed, device=device, plant_params=plant_params, tracks=tracks, track_id=track_id).run()


class SeedLaps(_Plant):
    """The two laps in front of the learning MPC, for B cars at once and per car, device-resident: every car drives lap 0 under PID and
    lap 1 under MPC-LTI from its own start state, with its own plant parameters and on its own controller model, and both laps become ITS
    safe set (tests/auto_racing_game_test.py:48-73: PID lap, MPC-LTI lap, add_trajectory(ego, 0), add_trajectory(ego, 1)).  The learning
    MPC's stage models are regressions over these laps, its terminal set is their points and its cost-to-go their step counts, so a fleet of
    different cars must not share them.  Per control step, without touching the host (include/crx.h "Seed laps", S1-S6):

        crx_cbf_solve_dev        zero obstacle slots = control.mpc_lti, masked: only the cars in their MPC-LTI lap solve
        crx_seed_commit_dev      the applied input: PID law, u_0 of the plan, or zero for a car that is done
        crx_plant_step_wrap_dev  plant + lap bookkeeping
        crx_seed_log_dev         a driving car logs the step and changes phase at the line; a seeded car is put back where it stood
        crx_lmpc_addtraj_dev     a car that crossed: its logged lap becomes a safe-set lap

    The cars finish at different steps; a car that has handed over (phase 2) stands at its hand-over state, so after run() xc / xg are
    the start states of every car's first learning-MPC lap and lmpc_inputs() is what LmpcLaps / GameLaps take -- device tensors, no host
    array in between.  vt, eyt: scalars or one value per car, the target of both laps (tests/auto_racing_game_test.py:122,131).  models =
    (A [B,6,6], B [B,6,2]), host arrays or device tensors (PidLaps.identify()): every car's MPC-LTI lap on its own model; A, B are then
    unused.  phase [B]: 0 PID lap, 1 MPC-LTI lap, 2 seeded, 3 failed; seed_status [B]: bit abi.CRX_SEED_MPC_FAILED = a step of the
    MPC-LTI lap applied an iterate that had not converged, abi.CRX_SEED_LOG_FULL = a lap did not reach the line within n_points - 1 steps."""

    def __init__(self, track_table, lap_length, track_width, A, B, xcurv0, xglob0, vt=0.7, eyt=0.0, N=10, n_points=600, n_laps=4, timestep=0.1,
                 device=None, noise_seed=None, models=None, plant_params=None, tracks=None, track_id=None):
        _one_track_only("SeedLaps", tracks, track_id)
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        Bn, P, L = self.batch, int(n_points), int(n_laps)
        if L < 2 or P < 2:
            raise ValueError("SeedLaps: two laps of safe set and two log rows at least (n_laps %d, n_points %d)" % (L, P))
        self.N, self.track_width = N, track_width
        if models is not None and A is None and B is None:   # (the descriptor's own model is not read then)
            A, B = np.zeros((6, 6)), np.zeros((6, 2))
        # control.mpc_lti's descriptor (control/control.py:71-76): MPCTrackingParam's weights, no obstacle slot
        self.desc = abi.cbf_desc(N, 0, A, B, Q=(10.0, 0.0, 0.0, 4.0, 0.0, 40.0), R=(0.1, 0.1), ey_max=track_width)
        self.vt, self.eyt = _per_race(vt, Bn, dev), _per_race(eyt, Bn, dev)
        self.xt = torch.zeros((Bn, 6), **f64)
        self.xt[:, 0], self.xt[:, 5] = self.vt, self.eyt
        self.ws = torch_api.CbfWorkspace(self.desc, Bn, dev)
        self.models = None if models is None else torch_api.CbfModels(self.desc, *_models(models[0], models[1], Bn, dev))
        self.obs_s, self.obs_e = torch.empty((Bn, 0, N + 1), **f64), torch.empty((Bn, 0, N + 1), **f64)
        self.lap_off, self.n_obs = torch.empty((Bn, 0), **f64), torch.zeros((Bn,), **i32)
        # the safe set as LMPCRacingGame.__init__ leaves it (utils/base.py:430-441), stored lap-major as LmpcLaps keeps it
        self.ss, self.us = torch.full((Bn, L, P, 6), 10000.0, **f64), torch.full((Bn, L, P, 2), 10000.0, **f64)
        self.qf = torch.zeros((Bn, L, P), **f64)
        self.time_ss, self.it = torch.full((Bn, L), 10000, **i32), torch.zeros((Bn,), **i32)
        self.pdesc = abi.lmpcprep_desc(12, P, L, self.tab.shape[0], timestep, lap_length)   # the hand-over reads n_points, n_laps, lap_length
        # the running lap as the simulator logs it, as in LmpcLaps
        self.log_x, self.log_u = torch.zeros((Bn, P, 6), **f64), torch.zeros((Bn, P, 2), **f64)
        self.log_x[:, 0] = self.xc
        self.n_log = torch.ones((Bn,), **i32)
        self.laps_prev, self.crossed = torch.zeros((Bn,), **i32), torch.zeros((Bn,), **i32)
        self.step_no, self.traj_status = torch.zeros((Bn,), **i32), torch.zeros((Bn,), **i32)
        self.phase, self.seed_status, self.m_mpc = torch.zeros((Bn,), **i32), torch.zeros((Bn,), **i32), torch.zeros((Bn,), **i32)
        self.u = torch.zeros((Bn, 2), **f64)
        self.k = 0

    def step(self):
        """One control step of every car, five libcrx launches: cbf_solve_dev (active = m_mpc), seed_commit_dev, plant_step_wrap_dev,
        seed_log_dev, lmpc_addtraj_dev (dispatch = "longest_first": one longest_first ahead of the solver launch)."""
        torch_api.cbf_solve_dev(self.desc, self.xc, self.xt, self.obs_s, self.obs_e, self.lap_off, self.n_obs, ws=self.ws, active=self.m_mpc,
                                order=_order(self, self.ws.iters, self.m_mpc), models=self.models)
        torch_api.seed_commit_dev(self.N, self.phase, self.vt, self.eyt, self.xc, self.ws.U, self.ws.status, self.seed_status, self.u)
        xc_prev, xg_prev = self.xc, self.xg
        self._advance(self.u, 2)
        torch_api.seed_log_dev(self.lap_length, xc_prev, xg_prev, self.xc, self.xg, self.u, self.laps, self.laps_prev, self.log_x, self.log_u,
                               self.n_log, self.crossed, self.phase, self.seed_status, self.m_mpc)
        torch_api.lmpc_addtraj_dev(self.pdesc, self.crossed, self.log_x, self.log_u, self.n_log, self.ss, self.us, self.qf, self.time_ss, self.it,
                                   self.step_no, self.xc, self.traj_status)
        self.k += 1

    def n_driving(self):
        """How many cars are still in their PID or MPC-LTI lap.  Synchronises: one count comes back from the device."""
        return int((self.phase < 2).sum())

    def run(self, max_steps, check_every=32):
        """step() until no car is in phase 0 or 1, max_steps at most.  One count is read from the device every check_every steps and
        nothing else returns to the host; the steps a finished batch takes until the next read change nothing (S4)."""
        while self.k < max_steps:
            self.step()
            if self.k % check_every == 0 and self.n_driving() == 0:
                break
        return self

    def lmpc_inputs(self, N=12):
        """What LmpcLaps / GameLaps are constructed from, by parameter name and as device tensors: the cars' safe sets and their hand-over
        states, and the linearisation points add_trajectory hands over from lap 0 (utils/base.py:651-653) for a learning MPC of horizon N.
        Nothing is read back here: a car whose phase is not 2 (check phase / seed_status) has no complete safe set, and a learning MPC
        started on it regresses over 10000-filled rows."""
        return dict(ss_xcurv=self.ss, u_ss=self.us, qfun=self.qf, time_ss=self.time_ss, it=self.it, xcurv0=self.xc, xglob0=self.xg,
                    lin_points=self.ss[:, 0, 1:N + 2], lin_input=self.us[:, 0, 1:N + 1])


def seed_laps(track_table, lap_length, track_width, A, B, xcurv0, xglob0, max_steps, vt=0.7, eyt=0.0, N=10, n_points=600, n_laps=4, timestep=0.1,
              device=None, noise_seed=None, models=None, plant_params=None, check_every=32):
    """SeedLaps run until every car has handed over (or max_steps): everything stays on the device (r.lmpc_inputs(), r.phase,
    r.seed_status)."""
    return SeedLaps(track_table, lap_length, track_width, A, B, xcurv0, xglob0, vt=vt, eyt=eyt, N=N, n_points=n_points, n_laps=n_laps,
                    timestep=timestep, device=device, noise_seed=noise_seed, models=models, plant_params=plant_params).run(max_steps, check_every)


class LqrLaps(_Plant):
    """B cars under the reference's LQR tracking controller (car_racing/tests/control_test.py --ctrl-policy lqr: one car under
    LQRTracking on its own), each on its own LTI model, device-resident.  The gain depends on the model only: ONE
    crx_lqr_design_dev in the constructor, then per control step ONE crx_lqr_step_dev (u = -K (x - xt)) and ONE
    crx_plant_step_wrap_dev.  A, B: one model (6,6), (6,2) for every car or per-car models [B,6,6], [B,6,2], host arrays or device
    tensors as PidLaps.identify() returns them.  A car whose design is CRX_SINGULAR (a failed fit's NaN model) has a NaN gain
    and drives NaN inputs: `design.status` says which."""

    def __init__(self, track_table, lap_length, xcurv0, xglob0, A, B, Q=np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0]), R=np.diag([0.1, 0.1]),
                 vt=0.8, eyt=0.0, max_iter=50, eps=0.01, timestep=0.1, device=None, noise_seed=None, plant_params=None, tracks=None,
                 track_id=None):
        dev = self._plant_init(track_table, lap_length, timestep, xcurv0, xglob0, noise_seed, device, plant_params, tracks, track_id)
        f64 = dict(dtype=torch.float64, device=dev)
        Bn = self.batch
        self.A, self.B = _models(A, B, Bn, dev)
        self.desc = abi.lqr_desc(Q=Q, R=R, max_iter=max_iter, eps=eps)
        self.xt = torch.zeros((Bn, 6), **f64)
        self.xt[:, 0], self.xt[:, 5] = _per_race(vt, Bn, dev), _per_race(eyt, Bn, dev)
        self.design = torch_api.lqr_design_dev(self.desc, self.A, self.B)
        self.K = self.design.K
        self.u = torch.zeros((Bn, 2), **f64)

    def step(self):
        """One control step of every car: lqr_step_dev, plant_step_wrap_dev."""
        torch_api.lqr_step_dev(self.K, self.xc, self.xt, self.u)
        self._advance(self.u, 2)


def lqr_laps(track_table, lap_length, xcurv0, xglob0, steps, A, B, Q=np.diag([10.0, 0.0, 0.0, 4.0, 0.0, 40.0]), R=np.diag([0.1, 0.1]),
             vt=0.8, eyt=0.0, max_iter=50, eps=0.01, timestep=0.1, device=None, noise_seed=None, log_every=1, plant_params=None, tracks=None,
             track_id=None):
    """xcurv0, xglob0 [B,6]; A, B as in LqrLaps; plant_params [B,10]: one car per row.  Returns host arrays: xcurv [T+1,B,6] (T = steps / log_every), u [T,B,2], K [B,2,6],
    design_status [B], design_iters [B], laps [B]."""
    r = LqrLaps(track_table, lap_length, xcurv0, xglob0, A, B, Q=Q, R=R, vt=vt, eyt=eyt, max_iter=max_iter, eps=eps, timestep=timestep,
                device=device, noise_seed=noise_seed, plant_params=plant_params, tracks=tracks, track_id=track_id)
    logs = _run_and_log(r.step, steps, log_every, dict(xcurv=lambda: r.xc, u=lambda: r.u))
    return dict(logs, K=r.K.cpu().numpy(),
                design_status=r.design.status.cpu().numpy(), design_iters=r.design.iters.cpu().numpy(), laps=r.laps.cpu().numpy())


class RaceStats:
    """Per-car race statistics of a closed loop, on the device (include/crx.h "Race statistics"): contacts, cars that left the track,
    lap times, overtakes made and suffered, samples under a flag, min clearance, max |ey| and the sums behind the RMS figures.
    Attaches to every loop of this module through its stats_inputs(); nothing here runs unless asked, and a loop without a RaceStats
    launches exactly what it launched before.

        st = RaceStats(loop)      # one reset launch
        st.update()               # sample 0: the initial states
        for k in range(steps):
            st.step()             # loop.step(), then ONE race_stats_dev: sample k + 1, the states after the step
        st.summary(), st.per_car()

    A sample shows the kernel the loop as it is at that moment: the states after the step against the scripted cars at the clock
    after the step (or the other cars of the race, same snapshot).  group [B] int32 in [0, n_groups) splits the summary.  All launches
    go to the current stream: construct and step a sub-batch's RaceStats under the stream the sub-batch runs on.  track_width
    overrides the loop's (the loops without a track width -- IlqrRaces, PidLaps, LqrLaps -- never count a car as off track without it).
    first_sample = 1: for a caller that takes no sample of the initial states, so that the sample after step k is still k + 1.
    Track sets: a FieldRaces / MixedRaces built with tracks= / race_track= is sampled through race_stats_laps_dev with the loop's car_lap
    (every car folded by its own track's lap length).  The per-car loops PidLaps, LqrLaps and MpccbfRaces with tracks= / track_id= are still
    refused -- crx_race_stats_laps_dev would serve them as well; lifting that is a follow-up."""

    def __init__(self, loop, group=None, n_groups=1, track_width=None, first_sample=0):
        self.loop = loop
        ts = getattr(getattr(loop, "lm", loop), "tracks", None)
        if ts is not None and getattr(ts, "race_track", None) is None:
            raise ValueError("RaceStats takes one lap length (crx_stats_desc): a loop on a track set (tracks=, one track per car) has one per car")
        # a field on one track per race (FieldRaces, MixedRaces with race_track=): every sample through race_stats_laps_dev with the cars' own
        # lap lengths; the descriptor carries track 0's only to be a valid one
        self.car_lap = None if ts is None else ts.car_lap
        inp = loop.stats_inputs()
        xc = inp["xcurv"]
        Bn, dev = xc.shape[0], xc.device
        n_cars = int(inp.get("n_cars") or 0)
        V = n_cars - 1 if n_cars else (inp["car_s0"].shape[1] if inp.get("car_s0") is not None else 0)
        if track_width is None:
            track_width = inp.get("track_width")
        self.desc = abi.stats_desc(V, n_cars, inp["lap_length"] if ts is None else float(ts.host.lap_length[0]),
                                   float("inf") if track_width is None else track_width,
                                   l_sum=inp.get("l_sum") or 0.4, w_sum=inp.get("w_sum") or 0.2)
        self.ws = torch_api.RaceStatsWorkspace(self.desc, Bn, dev)
        self.group, self.n_groups = None, int(n_groups)
        if group is not None:
            self.group = group.to(dtype=torch.int32, device=dev).contiguous() if torch.is_tensor(group) else _dev(group, dev, torch.int32)
        self.n_updates = int(first_sample)
        torch_api.race_stats_reset_dev(self.desc, inp["laps"], self.ws)

    def update(self):
        """ONE race_stats_dev (race_stats_laps_dev for a field on one track per race) on the current stream; the sample index is the
        number of updates so far."""
        inp = self.loop.stats_inputs()
        kw = dict(car_s0=inp.get("car_s0"), car_v=inp.get("car_v"), car_ey=inp.get("car_ey"), n_opp=inp.get("n_opp"), car_dims=inp.get("car_dims"),
                  xt=inp.get("xt"), flag=inp.get("flag"))
        if self.car_lap is None:
            torch_api.race_stats_dev(self.desc, self.n_updates, inp["t"], inp["xcurv"], inp["laps"], self.ws, **kw)
        else:
            torch_api.race_stats_laps_dev(self.desc, self.n_updates, inp["t"], inp["xcurv"], inp["laps"], self.ws, lap_length=self.car_lap, **kw)
        self.n_updates += 1

    def step(self):
        self.loop.step()
        self.update()

    def summary(self):
        """The host record(s) by field name (abi.STATS_SUM_I, abi.STATS_SUM_D; laps_hist: 9 bins): a dict, or with a group array a list
        of n_groups dicts.  Synchronises."""
        sum_i, sum_d = torch_api.race_stats_summary_dev(self.desc, self.ws, self.group, self.n_groups)
        sum_i, sum_d = sum_i.cpu().numpy(), sum_d.cpu().numpy()
        recs = [abi.stats_summary_record(sum_i[g], sum_d[g]) for g in range(sum_i.shape[0])]
        return recs if self.group is not None else recs[0]

    def per_car(self):
        """Host arrays by field name: [B] each, lap_step [8,B], ds_prev [n_opp_max,B].  Synchronises."""
        return {name: v.cpu().numpy() for name, v in self.ws.fields().items()}
