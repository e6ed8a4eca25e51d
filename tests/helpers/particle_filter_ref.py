"""NumPy restatement of mcl_3dl's filter step, float32 / float64 as the reference mixes them (citations relative to the
reference's src/dddmr_mcl_3dl/): pf.h's measure / expectation / expectationBiased / covariance / max / resample / noise,
state_6dof.h's operator+ / generateNoise / ParticleWeightedMeanQuat, quat.h, the differential-drive motion model, nd.h's
NormalLikelihood and the lambdas of src/mcl_3dl.cpp (bias :518-530, update_noise_func :221-229, integ_reset_func
:570-575).  Sums run in index order.  The transcendentals (sinf, cosf, acosf, expf) are the C library's own, called
through ctypes, since they are what the reference calls.  One deliberate difference, the library's: among equal
accum_probability_ values resample picks the lowest index (pf.h's std::sort orders equal keys as libstdc++'s introsort
leaves them once there are more than 16).

States are [N,13] float32 in State6DOF::operator[] order; noise4 rows are noise_ll_, noise_la_, noise_al_, noise_aa_;
noise rows are [*,10]: pos xyz, rot xyzw, odom_err_integ_ang_ xyz of the state generateNoise builds."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
D = np.float64

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "acosf", "expf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def _m(name, x):
    return F(getattr(_libm, name)(float(x)))


# ---- quat.h / vec3.h on float32 scalars and rows ----------------------------------------------------------------------
def qmul(a, b):
    """Quat::operator*(const Quat&); a, b [...,4] float32 (x y z w), every sum left to right"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1).astype(F)


def qdot(q):
    q = np.asarray(q, F)
    return (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]).astype(F)


def qscale_inv(q, s):
    """operator/(s): operator*(float(1.0 / s))"""
    r = (D(1.0) / np.asarray(s, F).astype(D)).astype(F)
    return (np.asarray(q, F) * r[..., None]).astype(F)


def qconj(q):
    q = np.asarray(q, F)
    return (q * np.array([-1, -1, -1, 1], F)).astype(F)


def qinv(q):
    return qscale_inv(qconj(q), qdot(q))


def qnormalized(q):
    return qscale_inv(q, np.sqrt(qdot(q)).astype(F))


def qrot(q, v):
    """Quat::operator*(const Vec3&) with the raw rotation"""
    q, v = np.asarray(q, F), np.asarray(v, F)
    p = np.concatenate([np.broadcast_to(v, q.shape[:-1] + (3,)), np.zeros(q.shape[:-1] + (1,), F)], axis=-1)
    return qmul(qmul(q, p), qconj(q))[..., :3]


def axis_angle(q):
    """Quat::getAxisAng's angle for one quaternion"""
    w = F(q[3])
    if abs(D(w)) >= 1.0 - 0.000001:
        return F(0.0)
    ang = F(D(_m("acosf", w)) * 2.0)
    if D(ang) > np.pi:
        ang = F(D(ang) - 2.0 * np.pi)
    return ang


def norm3(v):
    v = np.asarray(v, F)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]).astype(F)).astype(F)


def cross3(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def quat_from_axes(forward, up_raw):
    """Quat(const Vec3& forward, const Vec3& up_raw)"""
    with np.errstate(all="ignore"):
        forward, up_raw = np.asarray(forward, F), np.asarray(up_raw, F)
        xv = (forward / norm3(forward)).astype(F)
        c = cross3(up_raw, xv)
        yv = (c / norm3(c)).astype(F)
        c = cross3(xv, yv)
        zv = (c / norm3(c)).astype(F)

        def half_root(v):
            v = D(v)
            return F(np.sqrt(v if v > 0.0 else D(0.0)) / 2.0)
        x, y, z = D(xv[0]), D(yv[1]), D(zv[2])
        q = np.array([half_root(1.0 + x - y - z), half_root(1.0 - x + y - z), half_root(1.0 - x - y + z), half_root(1.0 + x + y + z)], F)
        if F(zv[1] - yv[2]) > 0:
            q[0] = -q[0]
        if F(xv[2] - zv[0]) > 0:
            q[1] = -q[1]
        if F(yv[0] - xv[1]) > 0:
            q[2] = -q[2]
        return q


def quat_from_rpy(rpy):
    """Quat::setRPY"""
    r = np.asarray(rpy, F)
    t2, t3 = _m("cosf", r[0] / F(2)), _m("sinf", r[0] / F(2))
    t4, t5 = _m("cosf", r[1] / F(2)), _m("sinf", r[1] / F(2))
    t0, t1 = _m("cosf", r[2] / F(2)), _m("sinf", r[2] / F(2))
    return np.array([t0 * t3 * t4 - t1 * t2 * t5, t0 * t2 * t5 + t1 * t3 * t4, t1 * t2 * t4 - t0 * t3 * t5, t0 * t2 * t4 + t1 * t3 * t5], F)


def noise_row(draws):
    """generateNoise with a zero mean: six DiagonalNoiseGenerator draws (x y z roll pitch yaw) -> a [10] noise row"""
    d = np.asarray(draws, F)
    return np.concatenate([d[:3], quat_from_rpy(d[3:6]), (d[3:6] - F(0)).astype(F)]).astype(F)


# ---- the motion model -------------------------------------------------------------------------------------------------
def set_odoms(odom_prev, odom_cur, time_diff, lin_tc, ang_tc):
    """setOdoms -> dict(rt [3], rq [4], rt_norm, rel_ang, decay_lin, decay_ang), all float32"""
    a, b = np.asarray(odom_prev, F), np.asarray(odom_cur, F)
    inv = qinv(a[3:7])
    rt = qrot(inv, (b[:3] - a[:3]).astype(F))
    rq = qmul(inv, b[3:7])
    td = F(time_diff)
    return dict(rt=rt, rq=rq, rt_norm=norm3(rt), rel_ang=axis_angle(rq),
                decay_lin=F(1.0 - D(F(td / F(lin_tc)))), decay_ang=F(1.0 - D(F(td / F(ang_tc)))))


def predict(states, noise4, o):
    """MotionPredictionModelDifferentialDrive::predict for every particle -> states [N,13]"""
    s, z = np.asarray(states, F), np.asarray(noise4, F)
    n = len(s)
    ll, la, al, aa = z[:, 0], z[:, 1], z[:, 2], z[:, 3]
    rt = o["rt"]
    s1 = (D(1.0) + ll.astype(D)).astype(F)
    zero = np.zeros(n, F)
    diff = np.stack([rt[0] * s1 + al * o["rel_ang"], rt[1] * s1 + zero, rt[2] * s1 + zero], axis=1).astype(F)
    rot = s[:, 3:7]
    lin = (s[:, 7:10] + (diff - rt[None, :]).astype(F)).astype(F)
    pos = (s[:, 0:3] + qrot(rot, diff)).astype(F)
    yaw = (la * o["rt_norm"] + aa * o["rel_ang"]).astype(F)
    half = (yaw / F(2)).astype(F)
    sn = np.array([_m("sinf", h) for h in half], F)
    cs = np.array([_m("cosf", h) for h in half], F)
    qz = qnormalized(np.stack([F(0) * sn, F(0) * sn, F(1) * sn, cs], axis=1).astype(F))
    r = qnormalized(qmul(qmul(qz, rot), np.broadcast_to(o["rq"], (n, 4))))
    ang = (s[:, 10:13] + np.stack([zero, zero, yaw], axis=1)).astype(F)
    out = np.empty((n, 13), F)
    out[:, 0:3], out[:, 3:7] = pos, r
    out[:, 7:10] = lin * o["decay_lin"]
    out[:, 10:13] = ang * o["decay_ang"]
    return out


def predict_f64(states, noise4, o):
    """the same evaluated in float64 throughout (the float32 plan `o` is an input), not rounded"""
    s, z = np.asarray(states, F).astype(D), np.asarray(noise4, F).astype(D)
    n = len(s)
    rt, rq = o["rt"].astype(D), o["rq"].astype(D)
    ll, la, al, aa = z[:, 0], z[:, 1], z[:, 2], z[:, 3]
    diff = rt[None, :] * (1.0 + ll)[:, None]
    diff[:, 0] += al * D(o["rel_ang"])

    def qm(a, b):
        ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
        bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
        return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                         aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)
    rot = s[:, 3:7]
    conj = rot * np.array([-1, -1, -1, 1.0])
    mv = qm(qm(rot, np.concatenate([diff, np.zeros((n, 1))], axis=1)), conj)[:, :3]
    yaw = la * D(o["rt_norm"]) + aa * D(o["rel_ang"])
    qz = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    r = qm(qm(qz, rot), np.broadcast_to(rq, (n, 4)))
    r = r / np.sqrt((r * r).sum(axis=1))[:, None]
    out = np.empty((n, 13), D)
    out[:, 0:3], out[:, 3:7] = s[:, 0:3] + mv, r
    out[:, 7:10] = (s[:, 7:10] + (diff - rt[None, :])) * D(o["decay_lin"])
    ang = s[:, 10:13].copy()
    ang[:, 2] += yaw
    out[:, 10:13] = ang * D(o["decay_ang"])
    return out


# ---- the bias ---------------------------------------------------------------------------------------------------------
def normal_likelihood(sigma):
    """NormalLikelihood<float>(sigma): (a_, sq2_)"""
    sg = F(sigma)
    return F(1.0 / np.sqrt(2.0 * np.pi * D(sg) * D(sg))), F(D(F(sg * sg)) * 2.0)


def bias(states, state_prev, var_dist, var_ang):
    """probability_bias_ of every particle (src/mcl_3dl.cpp:508-531); state_prev None: 1.0"""
    s = np.asarray(states, F)
    if state_prev is None:
        return np.ones(len(s), F)
    sp = np.asarray(state_prev, F)
    a_l, q_l = normal_likelihood(var_dist)
    a_a, q_a = normal_likelihood(var_ang)
    lin = norm3((s[:, 0:3] - sp[None, 0:3]).astype(F))
    q = qmul(s[:, 3:7], np.broadcast_to(qinv(sp[3:7]), (len(s), 4)))
    out = np.empty(len(s), F)
    for i in range(len(s)):
        ang = axis_angle(q[i])
        nl = F(a_l * _m("expf", F(F(-lin[i]) * lin[i]) / q_l))
        na = F(a_a * _m("expf", F(F(-ang) * ang) / q_a))
        out[i] = F(D(F(nl * na)) + 1e-6)
    return out


def bias_f64(states, state_prev, var_dist, var_ang):
    """the same in float64 throughout (the float32 constants and state_prev_.rot_.inv() are inputs), not rounded"""
    s, sp = np.asarray(states, F).astype(D), np.asarray(state_prev, F)
    a_l, q_l = (D(v) for v in normal_likelihood(var_dist))
    a_a, q_a = (D(v) for v in normal_likelihood(var_ang))
    inv = qinv(sp[3:7]).astype(D)
    d = s[:, 0:3] - sp[None, 0:3].astype(D)
    lin = np.sqrt((d * d).sum(axis=1))
    a, b = s[:, 3:7], inv
    w = a[:, 3] * b[3] - a[:, 0] * b[0] - a[:, 1] * b[1] - a[:, 2] * b[2]
    ang = np.where(np.abs(w) >= 1.0 - 0.000001, 0.0, np.arccos(np.clip(w, -1, 1)) * 2.0)
    ang = np.where(ang > np.pi, ang - 2.0 * np.pi, ang)
    return a_l * np.exp(-lin * lin / q_l) * a_a * np.exp(-ang * ang / q_a) + 1e-6


# ---- pf.h -------------------------------------------------------------------------------------------------------------
def weigh(prob, likelihood):
    """pf::measure -> (probability [N], weight_sum, restored)"""
    p, lk = np.asarray(prob, F), np.asarray(likelihood, F)
    prod = (p * lk).astype(F)
    total = F(0)
    for v in prod:
        total = F(total + v)
    if total > 0:
        return (prod / total).astype(F), total, 0
    return p.copy(), total, 1


def mean_terms(states, w):
    """ParticleWeightedMeanQuat::add's addends: [N,10] = w, pos * w, front * w, up * w"""
    s, w = np.asarray(states, F), np.asarray(w, F)
    front, up = qrot(s[:, 3:7], np.array([1, 0, 0], F)), qrot(s[:, 3:7], np.array([0, 0, 1], F))
    return np.concatenate([w[:, None], s[:, 0:3] * w[:, None], front * w[:, None], up * w[:, None]], axis=1).astype(F)


def ordered_sums(rows, limit=None):
    """float32 column sums in row order over the first `limit` rows"""
    acc = np.zeros(rows.shape[1], F)
    for r in rows[:limit]:
        acc = (acc + r).astype(F)
    return acc


def mean_from_sums(sums):
    """ParticleWeightedMeanQuat::getMean -> [7]"""
    with np.errstate(all="ignore"):
        return np.concatenate([(sums[1:4] / sums[0]).astype(F), quat_from_axes(sums[4:7], sums[7:10])]).astype(F)


def estimate(states, prob, bias_):
    """expectationBiased, max, covariance(1.0, 1.0) -> dict"""
    s, p, b = np.asarray(states, F), np.asarray(prob, F), np.asarray(bias_, F)
    n = len(s)
    sums_b = ordered_sums(mean_terms(s, (p * b).astype(F)))
    run, p_num = F(0), 0
    for v in p:                                  # expectation(1.0)'s break and covariance's p_num share the running sum
        run = F(run + v)
        p_num += 1
        if run > F(1.0):
            break
    sums_u = ordered_sums(mean_terms(s, p), p_num)
    e = mean_from_sums(sums_u)
    best, best_i = p[0], 0
    for i in range(n):
        if best < p[i]:
            best, best_i = p[i], i
    cov = np.zeros((6, 6), F)
    d = (s[:p_num, 0:6] - e[None, 0:6]).astype(F)
    with np.errstate(all="ignore"):
        for j in range(6):
            for k in range(j, 6):
                t = ((d[:, k] * d[:, j]).astype(F) * p[:p_num]).astype(F)
                acc = F(0)
                for v in t:
                    acc = F(acc + v)
                cov[j, k] = cov[k, j] = F(acc / sums_u[0])
    return dict(sums_biased=sums_b, sums=sums_u, mean_biased=mean_from_sums(sums_b), mean=e, p_num=p_num, max_index=best_i,
                max_state=s[best_i].copy(), cov=cov)


def add(state, row, normalize):
    """State6DOF::operator+ of one state [13] and a noise row [10] (+ normalize())"""
    s, z = np.asarray(state, F), np.asarray(row, F)
    out = np.empty(13, F)
    out[0:3] = s[0:3] + z[0:3]
    r = qmul(z[3:7], s[3:7])
    out[3:7] = qnormalized(r) if normalize else r
    out[7:10] = s[7:10] + z[0:3]
    out[10:13] = s[10:13] + z[7:10]
    return out


def resample(states, noise4, prob, u, rows):
    """resampleUsingNoiseGenerator with the lowest-index tie rule -> dict(states, noise4, probability, pick, row, n_duplicates,
    n_at_end, n_ties); rows may hold more rows than there are duplicates.  Fewer: None for the states (the call is refused)."""
    s, z, p = np.asarray(states, F), np.asarray(noise4, F), np.asarray(prob, F)
    n = len(s)
    accum = np.empty(n, F)
    acc, ties = F(0), 0
    for i in range(n):
        prev = acc
        acc = F(acc + p[i])
        ties += int(i > 0 and acc == prev)
        accum[i] = acc
    pstep = F(acc / F(n))
    initial_p = F(F(u) * pstep)
    pick, row = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    it = it_prev = 0
    n_dup = n_end = 0
    for i in range(n):
        pscan = F(F(pstep * F(i)) + initial_p)
        it = it + int(np.searchsorted(accum[it:], pscan, side="left"))
        if it == n:
            pick[i] = it_prev
            n_end += 1
            continue
        if it == it_prev:
            row[i] = n_dup
            n_dup += 1
        pick[i] = it
        it_prev = it
    out = dict(pick=pick, row=row, n_duplicates=n_dup, n_at_end=n_end, n_ties=ties, accum=accum,
               probability=np.full(n, F(1.0 / D(n)), F), states=None, noise4=None)
    rows = np.asarray(rows, F).reshape(-1, 10)
    if len(rows) < n_dup:
        return out
    ns, nz = s[pick].copy(), z[pick].copy()
    for i in np.nonzero(row >= 0)[0]:
        ns[i] = add(s[pick[i]], rows[row[i]], True)
        nz[i] = 0
    out["states"], out["noise4"] = ns, nz
    return out


def add_noise(states, rows):
    """pf::noise -> (states, noise4): every noise_* is 0 afterwards, as operator+'s default-constructed result has them"""
    s = np.asarray(states, F)
    return np.stack([add(s[i], rows[i], False) for i in range(len(s))]).astype(F), np.zeros((len(s), 4), F)
