"""Numpy model of crx_lmpc_prep and crx_lmpc_addpoint (include/crx.h, "Host work in front of the learning-MPC QP"), written from the
description there and from the formulas of the reference (control/lmpc_helper.py: compute_index, compute_Q_M, compute_b, the
unconstrained lmpc_loc_lin_reg, the linearisation of the Euler step at :130-189, select_points; utils/base.py add_point), plus the
seeded generators of the inputs that tests/test_lmpcprep_model_cpu.py and tests/test_gpu_lmpc_prep.py share.  It imports nothing from
the oracle or from libcrx; the descriptor is the plain class Desc below with the field names of crx_lmpcprep_desc.

What the model fixes, and how:
  distances   float64, one feature after the other, each abs((f - xl) * scale): the bits the kernel and the oracle get, so that "tie"
              means the same thing in all three.
  selection   inside = #(dist < bandwidth); inside >= max_neighbours: the max_neighbours first of a STABLE sort by distance, which is the
              order (distance, index) -- arm "top"; else everything inside -- arm "partial", or "empty" if that is nothing.  Selected
              samples are used in ascending index order, lap iter-2 before lap iter-1.
  regression  weights (1 - (dist / bandwidth)^2) 3/4 in float64; the two 5x5 normal systems M'KM w = M'K y over [vx vy wz u 1] (u = a for
              the vx row, delta for the vy and wz rows) formed and solved in numpy.longdouble, Gaussian elimination with partial
              pivoting.  A zero pivot is a singular stage: status 1, the stage's three regression rows keep what the caller passed.
  kinematics  rows 3..5 of A and C from the formulas of lmpc_helper.py:130-189, in float64, written out from the Euler step (kinematic_rows), with the one `den * 2`
              entry the reference has in the s row.
  safe set    per lap iter-1, iter-2: np.argmin (first minimum) of the 1-norm distance to x over ALL n_points rows, start row
              first + shift if that is >= 0, else first; n_ss_per_lap rows from there, rows past the end clamped to the last row.

prep_model() also returns a record of what ran, per (race, stage, lap): arm, tie (the k-th and the (k+1)-th smallest distance are equal),
tie_span (largest index distance within the group of samples AT the k-th distance), n, inside (samples within the bandwidth), count
(selected); per stage: total, distinct (different feature rows among the selected), cond_each (2-norm condition estimates of the two
normal matrices; inf if singular) and cond (the worse of the two); per (race, safe-set lap): first, near_tie (several rows at the
minimum), near_span, clamp (a row past the end was clamped), neg (first + shift < 0).  The generators return it with their inputs so that a test can assert what its inputs reach."""
import numpy as np

TOP, PARTIAL, EMPTY = 0, 1, 2
LD = np.longdouble


class Desc:
    """The fields of crx_lmpcprep_desc with its defaults (include/crx.h)."""

    def __init__(self, N, n_points, n_laps, n_seg, dt, lap_length, n_ss_per_lap=22, n_ss_laps=2, max_neighbours=40, shift=0,
                 bandwidth=5.0, scale=(0.1, 1.0, 1.0, 1.0, 1.0)):
        self.N, self.n_points, self.n_laps, self.n_seg, self.dt, self.lap_length = N, n_points, n_laps, n_seg, dt, lap_length
        self.n_ss_per_lap, self.n_ss_laps, self.max_neighbours, self.shift = n_ss_per_lap, n_ss_laps, max_neighbours, shift
        self.bandwidth, self.scale = bandwidth, tuple(scale)


# ---------------------------------------------------------------------------------------------------------------- model
def curvature(track, lap_length, s):
    """racing_env.get_curvature: s wrapped into one lap, the first segment with start <= s <= start + length."""
    while s > lap_length:
        s -= lap_length
    while s < 0.0:
        s += lap_length
    for row in track:
        if row[3] <= s <= row[3] + row[4]:
            return float(row[5])
    return 0.0


def distances(F, xl, scale):
    """Scaled 1-norm distance of every row of F [n,5] to xl, summed feature by feature in float64."""
    s = np.zeros(F.shape[0])
    for c in range(5):
        s = s + np.abs((F[:, c] - xl[c]) * scale[c])
    return s


def select(dist, bandwidth, k):
    """-> (ascending indices of the selected samples, arm, tie, tie_span)."""
    inside = int(np.count_nonzero(dist < bandwidth))
    if inside >= k:
        order = np.argsort(dist, kind="stable")
        dk = dist[order[k - 1]]
        tie = len(order) > k and dist[order[k]] == dk
        at = np.flatnonzero(dist == dk)
        return np.sort(order[:k]), TOP, bool(tie), int(at[-1] - at[0])
    idx = np.flatnonzero(dist < bandwidth)
    return idx, (PARTIAL if len(idx) else EMPTY), False, 0


def solve5(Q, rhs):
    """Gaussian elimination with partial pivoting in the type of Q; None if a pivot is zero or not finite."""
    Q, rhs = Q.copy(), rhs.copy()
    n = Q.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(Q[c:, c])))
        if not (np.abs(Q[p, c]) > 0) or not np.isfinite(Q[p, c]):
            return None
        if p != c:
            Q[[c, p]], rhs[[c, p]] = Q[[p, c]], rhs[[p, c]]
        for r in range(c + 1, n):
            f = Q[r, c] / Q[c, c]
            Q[r, c:] = Q[r, c:] - f * Q[c, c:]
            rhs[r] = rhs[r] - f * rhs[c]
    w = np.zeros_like(rhs)
    for r in range(n - 1, -1, -1):
        w[r] = (rhs[r] - Q[r, r + 1:] @ w[r + 1:]) / Q[r, r]
    return w


def _cond(Q):
    Q = np.asarray(Q, dtype=np.float64)
    if not np.isfinite(Q).all() or not Q.any():
        return np.inf
    with np.errstate(all="ignore"):
        sv = np.linalg.svd(Q, compute_uv=False)
    return float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf


def stage_selection(desc, ss_b, us_b, time_b, it, xl):
    """The samples a stage's regression uses: [(lap, indices, dist, arm, tie, tie_span, n, inside)] for lap iter-2, iter-1."""
    out = []
    for lapk in range(2):
        lap = it - 2 + lapk
        n = int(time_b[lap]) - 1
        F = np.hstack((ss_b[lap, :n, 0:3], us_b[lap, :n, :]))
        dist = distances(F, xl, desc.scale)
        idx, arm, tie, span = select(dist, desc.bandwidth, desc.max_neighbours)
        out.append((lap, idx, dist, arm, tie, span, n, int(np.count_nonzero(dist < desc.bandwidth))))
    return out


def regression(desc, ss_b, us_b, sel):
    """-> (rows [3,5] as float64 or None if singular, total, distinct, (cond of the vx system, of the vy / wz system)).
    Row r = coefficients of [vx vy wz u 1] for next-step vx (u = a), vy, wz (u = delta)."""
    Ma, Md, Y, K, Fall = [], [], [], [], []
    for lap, idx, dist, *_ in sel:
        r = dist[idx] / desc.bandwidth
        K.append((1.0 - r * r) * 3.0 / 4.0)
        one = np.ones((len(idx), 1))
        Ma.append(np.hstack((ss_b[lap, idx, 0:3], us_b[lap, idx, 1:2], one)))
        Md.append(np.hstack((ss_b[lap, idx, 0:3], us_b[lap, idx, 0:1], one)))
        Y.append(ss_b[lap, idx + 1, 0:3])
        Fall.append(np.hstack((ss_b[lap, idx, 0:3], us_b[lap, idx, :])))
    Ma, Md, Y, K, Fall = (np.concatenate(a).astype(LD) for a in (Ma, Md, Y, K, Fall))
    total = len(K)
    distinct = len(np.unique(Fall.astype(np.float64), axis=0)) if total else 0
    Qa, Qd = Ma.T @ (K[:, None] * Ma), Md.T @ (K[:, None] * Md)
    ba, bd = Ma.T @ (K[:, None] * Y[:, 0:1]), Md.T @ (K[:, None] * Y[:, 1:3])
    wa, wd = solve5(Qa, ba), solve5(Qd, bd)
    cond = (np.inf, np.inf) if wa is None or wd is None else (_cond(Qa), _cond(Qd))
    if wa is None or wd is None:
        return None, total, distinct, cond
    return np.stack((wa[:, 0], wd[:, 0], wd[:, 1])).astype(np.float64), total, distinct, cond


def kinematic_rows(x0, cur, dt):
    """Rows 3..5 of A and of C: the first-order expansion of one Euler step of (epsi, s, ey) about x0 = (vx, vy, wz, epsi, s, ey), with
    the curvature `cur` held constant:

        epsi+ = epsi + dt (wz - cur along / den)      along  = vx cos(epsi) - vy sin(epsi)    (speed along the centre line)
        s+    = s    + dt along / den                 across = vx sin(epsi) + vy cos(epsi)    (speed across it)
        ey+   = ey   + dt across                      den    = 1 - cur ey

    Gradients over the state: d along = (cos, -sin, 0, -across, 0, 0), d across = (sin, cos, 0, along, 0, 0), d (1 / den) = cur / den^2
    in ey.  Row = unit vector of the state + dt * gradient of the rate; offset = step(x0) - row . x0.
    ONE STATED DEVIATION, kept because the reference has it (lmpc_helper.py:163 in the kernel's comment): the ey entry of the s row is
    dt along cur / (2 den) there, where the derivative is dt along cur / den^2."""
    x0 = np.asarray(x0, dtype=np.float64)
    vx, vy, wz, epsi, s, ey = x0
    c, sn = np.cos(epsi), np.sin(epsi)
    along, across, den = vx * c - vy * sn, vx * sn + vy * c, 1.0 - cur * ey
    unit = np.eye(6)
    g_along, g_across = np.array([c, -sn, 0.0, -across, 0.0, 0.0]), np.array([sn, c, 0.0, along, 0.0, 0.0])
    g_s_rate = g_along / den                                             # of along / den, without its ey entry (set below)
    g_epsi_rate = unit[2] - cur * (g_s_rate + along * cur / den ** 2 * unit[5])
    rows = np.stack((unit[3] + dt * g_epsi_rate, unit[4] + dt * g_s_rate, unit[5] + dt * g_across))
    rows[1, 5] = dt * along * cur / (2.0 * den)                          # the stated deviation; dt along cur / den^2 otherwise
    step = np.array([epsi + dt * (wz - cur * along / den), s + dt * along / den, ey + dt * across])
    return rows, step - rows @ x0


def select_points(desc, ss_lap, qf_lap, x):
    """-> (points [6, n_ss_per_lap], cost-to-go [n_ss_per_lap], record)."""
    P = ss_lap.shape[0]
    norm = np.zeros(P)
    for k in range(6):
        norm = norm + np.abs(ss_lap[:, k] - x[k])
    first = int(np.argmin(norm))
    at = np.flatnonzero(norm == norm[first])
    neg = first + desc.shift < 0
    lo = first if neg else first + desc.shift
    rows = np.minimum(lo + np.arange(desc.n_ss_per_lap), P - 1)
    rec = dict(first=first, near_tie=len(at) > 1, near_span=int(at[-1] - at[0]), clamp=bool(lo + desc.n_ss_per_lap - 1 > P - 1), neg=bool(neg))
    return ss_lap[rows].T, qf_lap[rows], rec


def prep_model(desc, ss, us, qf, time_ss, it, x, lin_points, lin_input, track, from_plan=False, seed=None):
    """-> A [B,N,6,6], B [B,N,6,2], C [B,N,6], ss_sel [B,6,M], q_sel [B,M], status [B], record (module docstring).
    `seed` = (A, B, C) the outputs start from (zeros if None): a singular stage keeps its three regression rows."""
    Bn, N, M = len(it), desc.N, desc.n_ss_per_lap * desc.n_ss_laps
    A, Bm, C = (np.zeros((Bn, N, 6, 6)), np.zeros((Bn, N, 6, 2)), np.zeros((Bn, N, 6))) if seed is None else (np.array(a, dtype=np.float64) for a in seed)
    ss_sel, q_sel, status = np.zeros((Bn, 6, M)), np.zeros((Bn, M)), np.zeros(Bn, dtype=np.int32)
    rec = dict(arm=np.zeros((Bn, N, 2), dtype=int), tie=np.zeros((Bn, N, 2), dtype=bool), tie_span=np.zeros((Bn, N, 2), dtype=int),
               n=np.zeros((Bn, N, 2), dtype=int), count=np.zeros((Bn, N, 2), dtype=int), inside=np.zeros((Bn, N, 2), dtype=int), total=np.zeros((Bn, N), dtype=int),
               distinct=np.zeros((Bn, N), dtype=int), cond=np.zeros((Bn, N)), cond_each=np.zeros((Bn, N, 2)), singular=np.zeros((Bn, N), dtype=bool),
               first=np.zeros((Bn, desc.n_ss_laps), dtype=int), near_tie=np.zeros((Bn, desc.n_ss_laps), dtype=bool),
               near_span=np.zeros((Bn, desc.n_ss_laps), dtype=int), clamp=np.zeros((Bn, desc.n_ss_laps), dtype=bool),
               neg=np.zeros((Bn, desc.n_ss_laps), dtype=bool))
    for b in range(Bn):
        for i in range(N):
            ix, iu = (min(i + 1, N), min(i + 1, N - 1)) if from_plan else (i, i)
            x0, u0 = lin_points[b, ix], lin_input[b, iu]
            sel = stage_selection(desc, ss[b], us[b], time_ss[b], int(it[b]), np.concatenate((x0[0:3], u0)))
            for lapk, (_, idx, _, arm, tie, span, n, inside) in enumerate(sel):
                rec["arm"][b, i, lapk], rec["tie"][b, i, lapk], rec["tie_span"][b, i, lapk] = arm, tie, span
                rec["n"][b, i, lapk], rec["count"][b, i, lapk], rec["inside"][b, i, lapk] = n, len(idx), inside
            w, rec["total"][b, i], rec["distinct"][b, i], rec["cond_each"][b, i] = regression(desc, ss[b], us[b], sel)
            rec["cond"][b, i] = rec["cond_each"][b, i].max()
            if w is None:
                status[b], rec["singular"][b, i] = 1, True
            else:
                A[b, i, 0:3], Bm[b, i, 0:3] = 0.0, 0.0
                A[b, i, 0:3, 0:3] = w[:, 0:3]
                Bm[b, i, 0, 1], Bm[b, i, 1, 0], Bm[b, i, 2, 0] = w[0, 3], w[1, 3], w[2, 3]
                C[b, i, 0:3] = w[:, 4]
            Bm[b, i, 3:6] = 0.0
            A[b, i, 3:6], C[b, i, 3:6] = kinematic_rows(x0, curvature(track, desc.lap_length, float(x0[4])), desc.dt)
        for jj in range(desc.n_ss_laps):
            lap = int(it[b]) - jj - 1
            pts, q, r = select_points(desc, ss[b, lap], qf[b, lap], x[b])
            ss_sel[b, :, jj * desc.n_ss_per_lap:(jj + 1) * desc.n_ss_per_lap] = pts
            q_sel[b, jj * desc.n_ss_per_lap:(jj + 1) * desc.n_ss_per_lap] = q
            for k, v in r.items():
                rec[k][b, jj] = v
    return A, Bm, C, ss_sel, q_sel, status, rec


def predictions(A, B, C, lin_points, lin_input, from_plan=False):
    """What the three regression rows predict at each stage's own linearisation point: [B,N,3]."""
    N = A.shape[1]
    if from_plan:
        lin_points = np.concatenate((lin_points[:, 1:], lin_points[:, -1:]), axis=1)
        lin_input = np.concatenate((lin_input[:, 1:], lin_input[:, -1:]), axis=1)
    return (np.einsum("bnij,bnj->bni", A[:, :, 0:3], lin_points[:, :N]) + np.einsum("bnij,bnj->bni", B[:, :, 0:3], lin_input)
            + C[:, :, 0:3])


def well_posed(rec):
    """[B,N]: at least 10 selected samples and a condition estimate of at most 1e12."""
    return (rec["total"] >= 10) & (rec["cond"] <= 1e12)


def addpoint_model(desc, ss, us, time_ss, it, step, x, u, u_stride):
    """LMPCRacingGame.add_point with the kernel's bounds: row time_ss[iter-1] + step + 1 of lap iter-1 becomes x + lap_length in s and
    the input u[b * u_stride : b * u_stride + 2]; a lap or a row outside the arrays changes nothing.  -> (ss, us) copies."""
    ss, us, u = ss.copy(), us.copy(), np.asarray(u).reshape(-1)
    for b in range(len(it)):
        lap = int(it[b]) - 1
        if not 0 <= lap < desc.n_laps:
            continue
        row = int(time_ss[b, lap]) + int(step[b]) + 1
        if not 0 <= row < desc.n_points:
            continue
        ss[b, lap, row] = x[b] + np.array([0, 0, 0, 0, desc.lap_length, 0])
        us[b, lap, row] = u[b * u_stride:b * u_stride + 2]
    return ss, us


# ----------------------------------------------------------------------------------------------------------- generators
LAP_LENGTH = 19.25
TRACK = np.array([[0.0, 0.0, 0.0, s0, ln, cur] for s0, ln, cur in
                  ((0.0, 3.0, 0.0), (3.0, 2.0, 0.8), (5.0, 4.0, 0.0), (9.0, 2.5, -0.6), (11.5, 3.5, 0.5), (15.0, 4.25, 0.0))])


def make_laps(rng, Bn, L, P, time_ss, dup):
    """Smooth laps with noise on them: rows 0 .. time_ss-1 of every lap hold a lap, the rest a filler far from every lap.  A share
    `dup` of the feature rows (vx vy wz | delta a) of each lap is overwritten by the features of another row of the lap, whose next
    row differs: exact ties of distance from any query point.  qfun counts down to the end of the lap."""
    ss, us, qf = np.zeros((Bn, L, P, 6)), np.zeros((Bn, L, P, 2)), np.zeros((Bn, L, P))
    j = np.arange(P)
    for b in range(Bn):
        for lap in range(L):
            t = int(time_ss[b, lap])
            ph, fr = rng.uniform(0, 2 * np.pi, 8), rng.uniform(1.0, 5.0, 8)
            w = 2 * np.pi * j / t
            ss[b, lap, :, 0] = 1.2 + 0.3 * np.sin(fr[0] * w + ph[0]) + rng.uniform(-0.1, 0.1, P)
            ss[b, lap, :, 1] = 0.25 * np.sin(fr[1] * w + ph[1]) + rng.uniform(-0.12, 0.12, P)
            ss[b, lap, :, 2] = 0.3 * np.sin(fr[2] * w + ph[2]) + rng.uniform(-0.12, 0.12, P)
            ss[b, lap, :, 3] = 0.2 * np.sin(fr[3] * w + ph[3]) + rng.uniform(-0.02, 0.02, P)
            ss[b, lap, :, 4] = LAP_LENGTH * j / max(t - 1, 1)
            ss[b, lap, :, 5] = 0.3 * np.sin(fr[4] * w + ph[4]) + rng.uniform(-0.02, 0.02, P)
            us[b, lap, :, 0] = 0.3 * np.sin(fr[5] * w + ph[5]) + rng.uniform(-0.12, 0.12, P)
            us[b, lap, :, 1] = 0.3 * np.sin(fr[6] * w + ph[6]) + rng.uniform(-0.12, 0.12, P)
            qf[b, lap] = (t - 1 - j) + 0.25 * lap
            n = t - 1
            tgt = rng.choice(n, size=int(dup * n), replace=False)
            src = rng.integers(0, n, len(tgt))
            ss[b, lap, tgt, 0:3], us[b, lap, tgt] = ss[b, lap, src, 0:3], us[b, lap, src]
            ss[b, lap, t:], us[b, lap, t:], qf[b, lap, t:] = 70.0 + lap + 0.001 * j[t:, None], -9.0, -3.0 - lap
    return ss, us, qf


def _lin_point(rng, ss_b, us_b, time_b, it, kind, spread):
    """One linearisation point (x0 [6], u0 [2]): kind 0 on a stored sample, 1 midway between two consecutive ones, 2 a stored
    sample displaced by up to `spread` per feature, 3 far from all data."""
    lap = it - 2 + int(rng.integers(0, 2))
    j = int(rng.integers(0, int(time_b[lap]) - 2))
    f = np.concatenate((ss_b[lap, j, 0:3], us_b[lap, j]))
    if kind == 1:
        f = 0.5 * (f + np.concatenate((ss_b[lap, j + 1, 0:3], us_b[lap, j + 1])))
    elif kind == 2:
        f = f + rng.uniform(-spread, spread, 5)
    elif kind == 3:
        f = f + 400.0
    x0 = np.concatenate((f[0:3], [rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 1.3 * LAP_LENGTH), rng.uniform(-0.4, 0.4)]))
    return x0, f[3:5]


def make_case(seed, N, P, L, t_lo, t_hi, k, dup, Bn=16, bandwidth=5.0, time_ss=None, kinds=(0, 1, 2), spread=0.4, far=None,
              n_ss_per_lap=22, n_ss_laps=2, shift=0, name=""):
    """One call's inputs.  time_ss drawn from t_lo..t_hi unless given, iter from 2..L.  `far` = {race: stages} get a linearisation
    point far from all data (an empty set in both laps: a singular stage); every other stage is drawn again until it selects none or
    at least 8 different feature rows (between the two, whether elimination meets an exact zero is a matter of rounding)."""
    rng = np.random.default_rng(seed)
    desc = Desc(N, P, L, len(TRACK), 0.1, LAP_LENGTH, n_ss_per_lap, n_ss_laps, k, shift, bandwidth)
    if time_ss is None:
        time_ss = rng.integers(t_lo, t_hi + 1, (Bn, L))
    time_ss = np.asarray(time_ss, dtype=np.int32)
    it = (2 + np.arange(Bn) % (L - 1)).astype(np.int32)
    rng.shuffle(it)
    ss, us, qf = make_laps(rng, Bn, L, P, time_ss, dup)
    lin_points, lin_input = np.zeros((Bn, N + 1, 6)), np.zeros((Bn, N, 2))
    for b in range(Bn):
        for i in range(N + 1):
            is_far = far is not None and i in far.get(b, ())
            while True:
                x0, u0 = _lin_point(rng, ss[b], us[b], time_ss[b], int(it[b]), 3 if is_far else kinds[int(rng.integers(0, len(kinds)))], spread)
                if is_far:
                    break
                sel = stage_selection(desc, ss[b], us[b], time_ss[b], int(it[b]), np.concatenate((x0[0:3], u0)))
                rows = np.concatenate([np.hstack((ss[b, lap, idx, 0:3], us[b, lap, idx])) for lap, idx, *_ in sel])
                if len(rows) == 0 or len(np.unique(rows, axis=0)) >= 8:
                    break
            lin_points[b, i] = x0
            if i < N:
                lin_input[b, i] = u0
    # current state: near a stored row of the lap before the running one
    x = np.zeros((Bn, 6))
    for b in range(Bn):
        lap = int(it[b]) - 1
        x[b] = ss[b, lap, int(rng.integers(0, time_ss[b, lap]))] + rng.normal(0, 0.01, 6)
    return dict(name=name, desc=desc, args=(ss, us, qf, time_ss, it, x, lin_points, lin_input, TRACK), from_plan=False)


def with_plan(case):
    """The same inputs with lin_points / lin_input read as the previous plan (from_plan: shifted by one stage inside)."""
    c = dict(case)
    c["from_plan"], c["name"] = True, case["name"] + "-plan"
    return c


def case_a():
    return make_case(101, 5, 160, 4, 70, 150, 40, 0.30, name="a")


def case_b():
    return make_case(102, 7, 1100, 3, 700, 1090, 64, 0.30, name="b")


C_BANDWIDTH, C_SPREAD = 0.74, 0.25    # case c: the ball then holds 0..60 samples of a lap (asserted in tests/test_lmpcprep_model_cpu.py)


def case_c():
    rng = np.random.default_rng(103)
    far = {b: set(rng.choice(6, size=3, replace=False).tolist()) for b in range(5)}
    return make_case(103, 6, 160, 4, 70, 150, 40, 0.30, bandwidth=C_BANDWIDTH, kinds=(0, 1, 2, 2), spread=C_SPREAD, far=far, name="c")


def case_d():
    out = []
    for N in (2, 3):
        c = make_case(104 + N, N, 96, 2, 60, 95, 8, 0.30, name="d-N%d" % N)
        out += [c, with_plan(c)]
    return out


def case_e():
    """A short lap and a long one in both orders; the long one just under the 512-sample boundary of the register-keyed bisection,
    and exactly on it."""
    t = np.array([(20, 500), (500, 20), (513, 20), (20, 513), (500, 513), (513, 500)] * 3, dtype=np.int32)[:16]
    return make_case(107, 4, 520, 2, 0, 0, 40, 0.30, time_ss=t, name="e")


def case_f():
    """Safe-set selection only (N = 2): full tables (every row of a lap is data) with state rows duplicated more than 64 rows apart, x on
    a stored row, next to a duplicated row (two rows at exactly the same distance), near row 0 and beyond the last row."""
    out = []
    P, L, Bn = 300, 3, 16
    for c, (npl, nlaps, shift) in enumerate((a, b, s) for a in (1, 7, 22, 30) for b in (1, 2) for s in (-5, 0, 3)):
        case = make_case(200 + c, 2, P, L, P, P, 8, 0.0, Bn=Bn, n_ss_per_lap=npl, n_ss_laps=nlaps, shift=shift, name="f-%d-%d-%d" % (npl, nlaps, shift))
        ss, us, qf, time_ss, it, x, lp, li, tr = case["args"]
        rng = np.random.default_rng(300 + c)
        for b in range(Bn):
            for lap in range(L):           # duplicated state rows: gaps over 64, among them multiples of 64 (same lane) and lower lanes
                for lo in rng.choice(P - 200, size=6, replace=False):
                    ss[b, lap, lo + int(rng.choice((65, 100, 128, 130, 192)))] = ss[b, lap, lo]
            lap = int(it[b]) - 1
            kind = b % 4
            if kind == 0:
                x[b] = ss[b, lap, int(rng.integers(0, P))]
            elif kind == 1:               # next to a row that has a twin: both at exactly the same distance
                j = next(j for j in rng.permutation(P - 65) if (ss[b, lap, j + 65:] == ss[b, lap, j]).all(axis=1).any())
                x[b] = ss[b, lap, j] + rng.normal(0, 1e-4, 6)
            elif kind == 2:
                x[b] = ss[b, lap, int(rng.integers(0, 3))] + rng.normal(0, 1e-3, 6)
            else:
                x[b] = ss[b, lap, P - 1 - int(rng.integers(0, 3))] + np.array([0, 0, 0, 0, rng.uniform(0.0, 0.5), 0])
        out.append(case)
    return out


def all_cases():
    """{name: [calls]} for the cases a..f of the test table (g is a, b, a in one process: tests/test_gpu_lmpc_prep.py)."""
    return dict(a=[case_a()], b=[case_b()], c=[case_c()], d=case_d(), e=[case_e()], f=case_f())


def run_model(case, seed=None):
    return prep_model(case["desc"], *case["args"], from_plan=case["from_plan"], seed=seed)


def make_addpoint(seed, u_stride, Bn=64, P=40, L=3):
    """Inputs of add_point: iter 0 .. L+1, rows time_ss + step + 1 on P-2, P-1, P, negative and inside; inputs at stride u_stride."""
    rng = np.random.default_rng(seed)
    desc = Desc(4, P, L, len(TRACK), 0.1, LAP_LENGTH)
    time_ss = rng.integers(5, P - 5, (Bn, L)).astype(np.int32)
    it = (np.arange(Bn) % (L + 2)).astype(np.int32)
    rng.shuffle(it)
    ss, us = rng.normal(size=(Bn, L, P, 6)), rng.normal(size=(Bn, L, P, 2))
    step = np.zeros(Bn, dtype=np.int32)
    targets = (P - 2, P - 1, P, -1, -7, 0, 17)
    for b in range(Bn):
        lap = min(max(int(it[b]) - 1, 0), L - 1)
        step[b] = targets[(b // (L + 2)) % len(targets)] - 1 - time_ss[b, lap]
    x, u = rng.normal(size=(Bn, 6)), rng.normal(size=(Bn, u_stride))
    return dict(desc=desc, ss=ss, us=us, time_ss=time_ss, it=it, step=step, x=x, u=u, u_stride=u_stride)
