"""Host-side mirror of Optimizer::InertialOptimization (src/Optimizer.cc:3469-3925) on the device
(openmavis_amd/csrc/inertial.hip): IMU initialisation for a batch of independent maps ("jobs") in one call.

    opt = InertialOptimizer(max_jobs, max_kf_total, max_edges_total)
    out = InertialOptimization(jobs, optimizer=opt)              # each job in its own mode
    out = InertialOptimization(jobs, mode=FULL, mono=True, priorG=1e2, priorA=1e5)   # (pMap, Rwg, scale, bg, ba, bMono, ..)
    out = InertialOptimization(jobs, mode=BIAS, priorG=1.0, priorA=1e5)              # (pMap, bg, ba, priorG, priorA)
    out = InertialOptimization(jobs, mode=GS)                                        # (pMap, Rwg, scale)

A job is a dict: Rwb [K][9], twb [K][3] (body poses, double: ImuCamPose of the keyframes), vel [K][3] (double),
old_bg [K][3] (float32: the keyframes' gyro bias before the call), kf1 / kf2 [E] (previous, current keyframe of every
EdgeInertialGS, indices into the job's keyframes), preint [E][292] (float32 records), bg0 / ba0 [3] (the bias of
vpKFs.front(): every bias vertex starts there), Rwg [9], scale, mode, mono, priorG, priorA.  select_edges() restates the
reference's edge tests, initial_guess() the start values of LocalMapping::InitializeIMU, reintegrate() what
Preintegrated::Reintegrate does to the flagged records.  There is no CPU fallback."""
import ctypes

import numpy as np

from . import _lib

FULL, BIAS, GS = 0, 1, 2          # OMV_INERTIAL_FULL / _BIAS / _GS
MAX_KF = 320                      # OMV_INERTIAL_MAX_KF: keyframes per job
PREINT_FLOATS = 292


def select_edges(prev, kf_id, is_bad, max_kf_id):
    """The edge tests of :3571-3594 on arrays over vpKFs: prev [n] the position of mPrevKF in vpKFs or -1, kf_id [n] mnId,
    is_bad [n].  Keyframes with mnId > maxKFid are no vertices.  Returns (keep [K] positions of the vertices, kf1, kf2 [E]
    as indices into keep)."""
    prev, kf_id, is_bad = np.asarray(prev, np.int64), np.asarray(kf_id, np.int64), np.asarray(is_bad, bool)
    keep = np.nonzero(kf_id <= max_kf_id)[0]
    where = -np.ones(len(prev), np.int64)
    where[keep] = np.arange(len(keep))
    k1, k2 = [], []
    for i in range(len(prev)):
        if prev[i] >= 0 and kf_id[i] <= max_kf_id:
            if is_bad[i] or kf_id[prev[i]] > max_kf_id:
                continue
            k1.append(where[prev[i]])
            k2.append(where[i])
    return keep, np.array(k1, np.int32), np.array(k2, np.int32)


def _so3f_exp(w):
    """Sophus::SO3f::exp(w).matrix() in float32."""
    f = np.float32
    w = np.asarray(w, f)
    th2 = f(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th2 < f(1e-5) * f(1e-5):
        imag, real = f(0.5) - f(1.0 / 48.0) * th2, f(1.0) - f(1.0 / 8.0) * th2
    else:
        th = f(np.sqrt(th2))
        half = f(0.5) * th
        imag, real = f(np.sin(half)) / th, f(np.cos(half))
    q = np.array([imag * w[0], imag * w[1], imag * w[2], real], f)
    x, y, z, r = q
    two = f(2)
    return np.array([[1 - two * (y * y + z * z), two * (x * y - z * r), two * (x * z + y * r)],
                     [two * (x * y + z * r), 1 - two * (x * x + z * z), two * (y * z - x * r)],
                     [two * (x * z - y * r), two * (y * z + x * r), 1 - two * (x * x + y * y)]], f)


def initial_guess(job):
    """The start of LocalMapping::InitializeIMU for a map that is not yet IMU-initialised (src/LocalMapping.cc:1300-1329),
    in float32: per edge, in edge order, dirG -= Rwb(prev) * GetUpdatedDeltaVelocity() (the records' own bias: the stored
    dV) and the velocity (p - p_prev) / dT set on both keyframes; Rwg = exp(gI x dirG * acos(gI . dirG) / |gI x dirG|).
    Returns dict(vel [K][3] float64 (float values), Rwg [3][3] float64)."""
    f = np.float32
    Rwb = np.asarray(job["Rwb"], np.float64).reshape(-1, 3, 3).astype(f)
    twb = np.asarray(job["twb"], np.float64).reshape(-1, 3).astype(f)
    pre = np.asarray(job["preint"], f).reshape(-1, PREINT_FLOATS)
    vel = np.zeros((len(Rwb), 3), f)
    dirG = np.zeros(3, f)
    for e, (a, b) in enumerate(zip(np.asarray(job["kf1"]).reshape(-1), np.asarray(job["kf2"]).reshape(-1))):
        dirG = (dirG - Rwb[a] @ pre[e, 9:12]).astype(f)
        v = ((twb[b] - twb[a]) / pre[e, 66]).astype(f)
        vel[b], vel[a] = v, v
    Rwg = np.eye(3, dtype=f)
    n = f(np.linalg.norm(dirG))
    if n > 0:
        dirG = (dirG / n).astype(f)
        gI = np.array([0, 0, -1], f)
        v = np.cross(gI, dirG).astype(f)
        nv = f(np.linalg.norm(v))
        ang = f(np.arccos(np.clip(f(gI @ dirG), f(-1), f(1))))
        if nv > 0:
            Rwg = _so3f_exp((v * ang / nv).astype(f))
    return dict(vel=vel.astype(np.float64), Rwg=Rwg.astype(np.float64))


class InertialOptimizer:
    """One omv_inertial_opt handle: up to max_jobs jobs, max_kf_total keyframes and max_edges_total edges per call (at
    most MAX_KF keyframes in one job)."""

    def __init__(self, max_jobs=8, max_kf_total=512, max_edges_total=512, stream=None):
        self._lib, self.stream = _lib.load(), stream
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.omv_inertial_opt_create(int(max_jobs), int(max_kf_total), int(max_edges_total),
                                                     ctypes.byref(self._h)), "omv_inertial_opt_create")
        self.K = np.zeros(0, np.int32)
        self.E = np.zeros(0, np.int32)

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.omv_inertial_opt_destroy(self._h)
            self._h = ctypes.c_void_p()

    def _stream(self):
        if self.stream is not None:
            return ctypes.c_void_p(self.stream.cuda_stream)
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def pack(jobs):
        """The call's arrays from the job dicts (also what tests/cpp/inertial_opt_consumer.cpp reads)."""
        J = len(jobs)
        K = np.array([len(np.asarray(j["Rwb"]).reshape(-1, 9)) for j in jobs], np.int32)
        E = np.array([len(np.asarray(j["kf1"]).reshape(-1)) for j in jobs], np.int32)

        def cat(key, dt, width):
            if not J:
                return np.zeros((0, width), dt)
            return np.ascontiguousarray(np.concatenate([np.asarray(j[key], dt).reshape(-1, width) for j in jobs]))

        a = dict(kf_start=np.concatenate([[0], np.cumsum(K)]).astype(np.int32),
                 edge_start=np.concatenate([[0], np.cumsum(E)]).astype(np.int32),
                 Rwb=cat("Rwb", np.float64, 9), twb=cat("twb", np.float64, 3), vel_in=cat("vel", np.float64, 3),
                 old_bg=cat("old_bg", np.float32, 3), kf1=cat("kf1", np.int32, 1), kf2=cat("kf2", np.int32, 1),
                 preint=cat("preint", np.float32, PREINT_FLOATS), bg0=cat("bg0", np.float64, 3),
                 ba0=cat("ba0", np.float64, 3), mode=cat("mode", np.int32, 1), mono=cat("mono", np.int32, 1),
                 priorG=cat("priorG", np.float32, 1), priorA=cat("priorA", np.float32, 1),
                 Rwg=cat("Rwg", np.float64, 9), scale=cat("scale", np.float64, 1))
        return a, K, E

    _IN = ("kf_start", "edge_start", "Rwb", "twb", "vel_in", "old_bg", "kf1", "kf2", "preint", "bg0", "ba0", "mode", "mono",
           "priorG", "priorA")

    def run(self, jobs):
        """omv_inertial_optimization on `jobs`; returns (status code, dict of the outputs over the whole call)."""
        a, K, E = self.pack(jobs)
        J, Kt = len(jobs), int(K.sum())
        o = dict(Rwg=a["Rwg"].copy(), scale=a["scale"].copy(), bg=np.zeros((max(J, 1), 3)), ba=np.zeros((max(J, 1), 3)),
                 vel=np.zeros((max(Kt, 1), 3)), vel_f32=np.zeros((max(Kt, 1), 3), np.float32),
                 reintegrate=np.zeros(max(Kt, 1), np.uint8), iterations=np.zeros(max(J, 1), np.int32),
                 trials=np.zeros(max(J, 1), np.int32))
        if J == 0:
            o["Rwg"], o["scale"] = np.zeros((1, 9)), np.zeros((1, 1))
        code = self._lib.omv_inertial_optimization(self._h, J, *[_lib.ptr(a[k]) for k in self._IN],
                                                   *[_lib.ptr(v) for v in o.values()], self._stream())
        if code == _lib.OMV_OK:
            self.K, self.E = K, E
        o["kf_start"], o["edge_start"] = a["kf_start"], a["edge_start"]
        return code, o

    def debug(self, j):
        """The library's test hook for job j of the last run, in the job's own keyframe and edge order: e0 [E][9] the
        residuals at the input state; the first system as Hvv [K][3][3] (velocity diagonal blocks), Hvoff [E][3][3] (V1
        rows, V2 columns of every edge), border [K][3][9] (velocity rows; columns bg ba gdir scale), bv [K][3],
        corner [9][9], bc [9], chi2, lambda_init; the first trial's xv [K][3], xc [9]; iterations, trials, max_trials;
        err [2] (GS: the float robust chi2 before and after); ticks [3] (100 MHz device clock: buildSystem, the linear
        solves, the trials' error evaluations)."""
        K, E = int(self.K[j]), int(self.E[j])
        o = dict(e0=np.zeros((max(E, 1), 9)), Hvv=np.zeros((max(K, 1), 3, 3)), Hvoff=np.zeros((max(E, 1), 3, 3)),
                 border=np.zeros((max(K, 1), 3, 9)), bv=np.zeros((max(K, 1), 3)), corner=np.zeros((9, 9)), bc=np.zeros(9),
                 chi2=np.zeros(1), lambda_init=np.zeros(1), xv=np.zeros((max(K, 1), 3)), xc=np.zeros(9),
                 iterations=np.zeros(1, np.int32), trials=np.zeros(1, np.int32), max_trials=np.zeros(1, np.int32),
                 err=np.zeros(2, np.float32), ticks=np.zeros(3, np.int64))
        _lib.check(self._lib.omv_inertial_opt_debug(self._h, int(j), *[_lib.ptr(v) for v in o.values()], self._stream()),
                   "omv_inertial_opt_debug")
        for k in ("e0", "Hvoff"):
            o[k] = o[k][:E]
        for k in ("Hvv", "border", "bv", "xv"):
            o[k] = o[k][:K]
        for k in ("chi2", "lambda_init"):
            o[k] = float(o[k][0])
        for k in ("iterations", "trials", "max_trials"):
            o[k] = int(o[k][0])
        return o


def InertialOptimization(jobs, mode=None, mono=None, priorG=None, priorA=None, optimizer=None):
    """Optimizer::InertialOptimization for every job in one device call.  mode / mono / priorG / priorA given here
    override the jobs' own (the reference's three call shapes).  Returns per job a dict: Rwg [3][3], scale, bg, ba [3],
    vel [K][3] (double), vel_f32 (what SetVelocity stores), reintegrate [K] (records to pass to reintegrate()),
    iterations, trials.  mode == GS writes only Rwg and scale; bg, ba and vel are the job's own."""
    jobs = [dict(j) for j in jobs]
    for j in jobs:
        for k, v in (("mode", mode), ("mono", mono), ("priorG", priorG), ("priorA", priorA)):
            if v is not None:
                j[k] = v
        j.setdefault("mono", 0), j.setdefault("priorG", 0.0), j.setdefault("priorA", 0.0)
        j.setdefault("Rwg", np.eye(3)), j.setdefault("scale", 1.0)
    nK = sum(len(np.asarray(j["Rwb"]).reshape(-1, 9)) for j in jobs)
    nE = sum(len(np.asarray(j["kf1"]).reshape(-1)) for j in jobs)
    opt = optimizer if optimizer is not None else InertialOptimizer(max(len(jobs), 1), max(nK, 1), max(nE, 1))
    code, o = opt.run(jobs)
    _lib.check(code, "omv_inertial_optimization")
    out = []
    for i in range(len(jobs)):
        k0, k1 = int(o["kf_start"][i]), int(o["kf_start"][i + 1])
        out.append(dict(Rwg=o["Rwg"][i].reshape(3, 3).copy(), scale=float(o["scale"][i, 0]), bg=o["bg"][i].copy(),
                        ba=o["ba"][i].copy(), vel=o["vel"][k0:k1].copy(), vel_f32=o["vel_f32"][k0:k1].copy(),
                        reintegrate=o["reintegrate"][k0:k1].copy(), iterations=int(o["iterations"][i]),
                        trials=int(o["trials"][i])))
    return out


def reintegrate(pre, records, bias, meas, start, stream=None):
    """Preintegrated::Reintegrate (src/ImuTypes.cc:152-158) for the records `records` (indices) of the PreintegratedBatch
    `pre`: Initialize(bu) -- here the new bias [6] (bax bay baz bwx bwy bwz) of the call -- and every stored measurement
    integrated again.  meas (device float32 [m][7]) / start (host int [n + 1]) are the batch's measurements.  Returns a new
    PreintegratedBatch holding the re-integrated records, in the order of `records`; pre.rec is updated in place too."""
    import torch
    from .imu import PreintegratedBatch
    records = np.asarray(records, np.int64).reshape(-1)
    start = np.asarray(start, np.int64)
    sub = PreintegratedBatch(len(records), pre.calib, device=pre.rec.device)
    sub.Initialize(np.tile(np.asarray(bias, np.float32).reshape(1, 6), (len(records), 1)))
    if len(records) == 0:
        return sub
    n = start[records + 1] - start[records]
    idx = np.concatenate([np.arange(start[r], start[r + 1]) for r in records]) if n.sum() else np.zeros(0, np.int64)
    m = meas[torch.as_tensor(idx, device=meas.device)].contiguous()
    st = torch.as_tensor(np.concatenate([[0], np.cumsum(n)]).astype(np.int32), device=meas.device)
    sub.IntegrateNewMeasurements(m, st, stream)
    pre.rec[torch.as_tensor(records, device=pre.rec.device)] = sub.rec
    pre.avg[torch.as_tensor(records, device=pre.rec.device)] = sub.avg
    return sub
