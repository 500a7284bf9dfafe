"""Host-side mirror of Optimizer::LocalInertialBA's optimisation (src/Optimizer.cc:2728-3385) on the
device LM of libomv_hip.so (openmavis_amd/csrc/lba.hip).

The reference builds a g2o graph from the local window (:2740-3267: VertexPose / VertexVelocity /
VertexGyroBias / VertexAccBias, EdgeInertial + EdgeGyroRW + EdgeAccRW per keyframe pair, EdgeMono per
observation) and runs `optimizer.optimize(opt_it)` with Levenberg-Marquardt (:3270-3274), then the
outlier test (:3282-3296) and the FAIL guard (:3317-3321).  Here the flattened graph is a problem dict
(see openmavis_amd.synth_ba.make_lba_problem for the field list, which is omv_lba_problem's):

    ba = LocalInertialBA(max_kf=64, max_cams=5, max_pts=40000, max_mono=300000, max_imu=64)
    ba.set_problem(prob)
    res, state = ba.optimize(opt_it=10, lambda_init=1.0, large=False)

`res` carries err / err_end (activeRobustChi2 before/after, as floats like the reference), status
(OMV_LBA_OK / OMV_LBA_FAIL), the LM iteration / trial counts and per-edge chi2 + outlier flags; `state`
the optimised Rwb, twb, Rcw, tcw, vel, bg, ba, pts.  There is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib
from .synth_ba import as_struct, read_state

OMV_LBA_OK = 0
OMV_LBA_FAIL = 1


def lba_options(large):
    """LocalInertialBA's LM settings: bLarge -> 4 iterations, user lambda 1e-2; else 10 and 1e0."""
    return dict(opt_it=4, lambda_init=1e-2) if large else dict(opt_it=10, lambda_init=1e0)


class _BlockSolverHandle:
    """What the handles on the block LDL^T solver share (LocalInertialBA, LocalBundleAdjustment, FullInertialBA,
    EssentialGraph): a subclass names its symbol prefix and sets _lib, _h and, with a problem, _s."""

    _PREFIX = None   # "omv_lba": omv_lba_destroy, omv_lba_debug_solve, ...
    _h = _s = None

    def _call(self, name, *args):
        sym = f"{self._PREFIX}_{name}"
        _lib.check(getattr(self._lib, sym)(self._h, *args), sym)

    def __del__(self):
        if self._h:
            getattr(self._lib, f"{self._PREFIX}_destroy")(self._h)
            self._h = None

    def _need(self, what):
        if self._s is None:
            raise _lib.OmvError(f"{type(self).__name__}.{what}: no problem set")

    def _read_solve(self, call, nb, n_plan):
        """debug_solve's result for `nb` blocks and a plan of `n_plan` entries; call(S, rhs, x, fail, plan, n_plan)
        is the handle's omv_*_debug_solve behind its own leading arguments."""
        n = 16 * nb
        S, rhs, x = np.zeros((n, n)), np.zeros(n), np.zeros(n)
        plan = np.full(n_plan, -1, np.int32)
        fail = ctypes.c_int(-1)
        call(_lib.ptr(S), _lib.ptr(rhs), _lib.ptr(x), ctypes.byref(fail), _lib.ptr(plan), len(plan))
        n_lev = int(plan[3])
        return dict(S=S, rhs=rhs, x=x, fail=fail.value, mode=int(plan[0]), n_slots=int(plan[1]), n_lds=int(plan[2]),
                    n_lev=n_lev, cols=[int(v) for v in plan[4:4 + n_lev]])


class _StagedBA(_BlockSolverHandle):
    """The three bundle adjustments (omv_lba and its kinds omv_vba, omv_fiba): the stage events of their LM step.  The
    pose graphs time a whole optimize() instead (EssentialGraph.last_ms)."""

    def enable_timing(self, on=True):
        """Per-stage events on the next optimize() calls (direct launches instead of the captured LM step)."""
        self._call("enable_timing", int(bool(on)))
        return self

    def stage_ms(self):
        """Device ms of the last optimize: build, schur, solve, update+errors; and the trial count."""
        ms = np.zeros(4)
        t = ctypes.c_int(0)
        self._call("stage_ms", _lib.ptr(ms), ctypes.byref(t))
        return dict(build=ms[0], schur=ms[1], solve=ms[2], update=ms[3], trials=t.value)


class LocalInertialBA(_StagedBA):
    """`rank`, `world`, `allreduce`: landmark sharding (omv_lba_set_comm).  Every rank
    passes the same full problem; `allreduce(ptr, count, stream)` sums `count` doubles of device
    memory in place over the ranks (openmavis_amd.dist.LbaAllReduce).  After optimize() a rank's
    result holds its own landmarks / edges (`shard()` names them) and every keyframe."""

    _PREFIX = "omv_lba"

    def __init__(self, max_kf=64, max_cams=5, max_pts=40000, max_mono=400000, max_imu=64, rank=0, world=1,
                 allreduce=None):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.omv_lba_create(max_kf, max_cams, max_pts, max_mono, max_imu, ctypes.byref(h)),
                   "omv_lba_create")
        self._lib, self._h = lib, h
        self._s = None
        self._keep = None
        self._cb = None
        if world > 1 and allreduce is None:
            raise ValueError("LocalInertialBA: world > 1 needs an allreduce")
        if allreduce is not None:   # a collective given: the sharded call sequence, also on one rank

            def _cb(_ctx, buf, count, stream):
                try:
                    allreduce(buf, count, stream)
                    return 0
                except Exception as exc:   # reported by the failing omv_lba_optimize status
                    print(f"LocalInertialBA allreduce failed: {exc!r}")
                    return 1
            self._cb = _lib.ALLREDUCE_FN(_cb)
            _lib.check(lib.omv_lba_set_comm(h, int(rank), int(world), ctypes.cast(self._cb, ctypes.c_void_p), None),
                       "omv_lba_set_comm")

    def set_problem(self, prob):
        s, keep = as_struct(prob, _lib.LbaProblem)
        _lib.check(self._lib.omv_lba_set_problem(self._h, ctypes.byref(s)), "omv_lba_set_problem")
        self._s, self._keep = s, keep
        return self

    def optimize(self, opt_it=10, lambda_init=1e0, max_trials=10, large=False, chi2=True, state_copy=True):
        """chi2=False: only the outlier flags (what the reference's culling uses), no per-edge chi2 read-back.
        The optimised state is written back into the problem's host arrays (as the reference writes its keyframes and
        map points); state_copy=False returns those arrays themselves instead of copies (the next optimize() of this
        problem overwrites them)."""
        self._need("optimize")
        o = _lib.LbaOpts(int(opt_it), float(lambda_init), int(max_trials), int(bool(large)))
        E, S = self._s.n_mono, self._s.n_stereo
        want = bool(chi2)
        chi2 = np.zeros(E) if want else None
        outl = np.zeros(E, np.uint8)
        s_chi2 = np.zeros(S) if want else None
        s_outl = np.zeros(S, np.uint8)
        r = _lib.LbaResult()
        r.mono_chi2, r.mono_outlier = (_lib.ptr(chi2) if want else None), _lib.ptr(outl)
        r.stereo_chi2, r.stereo_outlier = (_lib.ptr(s_chi2) if want else None), _lib.ptr(s_outl)
        _lib.check(self._lib.omv_lba_optimize(self._h, ctypes.byref(o), ctypes.byref(self._s), ctypes.byref(r)),
                   "omv_lba_optimize")
        res = dict(err=r.err, err_end=r.err_end, status=r.status, iterations=r.iterations, trials=r.trials,
                   lambda_=r.lambda_, mono_chi2=chi2, mono_outlier=outl, stereo_chi2=s_chi2, stereo_outlier=s_outl)
        if not state_copy:
            return res, {k: self._keep[k] for k in ("Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba", "pts")}
        return res, read_state(self._keep)

    def reset(self):
        """Restore the state uploaded by set_problem (device copy)."""
        _lib.check(self._lib.omv_lba_reset(self._h), "omv_lba_reset")
        return self

    def evaluate(self):
        """Residuals and visual Jacobians at the uploaded state (caller's edge order)."""
        E, I = self._s.n_mono, self._s.n_imu
        me, jx, jp, ie = np.zeros((E, 2)), np.zeros((E, 6)), np.zeros((E, 12)), np.zeros((I, 9))
        _lib.check(self._lib.omv_lba_evaluate(self._h, _lib.ptr(me), _lib.ptr(jx), _lib.ptr(jp), _lib.ptr(ie)),
                   "omv_lba_evaluate")
        S = self._s.n_stereo
        se, sx, sp = np.zeros((S, 3)), np.zeros((S, 9)), np.zeros((S, 18))
        _lib.check(self._lib.omv_lba_evaluate_stereo(self._h, _lib.ptr(se), _lib.ptr(sx), _lib.ptr(sp)),
                   "omv_lba_evaluate_stereo")
        return dict(mono_err=me, mono_jx=jx, mono_jp=jp, imu_err=ie, stereo_err=se, stereo_jx=sx, stereo_jp=sp)

    def debug_solve(self, lambda_):
        """One reduced-system solve at the uploaded state with damping `lambda_` (omv_lba_debug_solve; a test hook):
        S [n][n] dense in keyframe order (n = 16 n_opt, padding rows included), rhs [n], x [n], the fail flag and the
        solver's plan: mode (1 all blocks in LDS, 2 hybrid, 0 global), n_slots, n_lds, n_lev, cols (per level)."""
        self._need("debug_solve")
        o = _lib.LbaOpts(10, 1e0, 10, 0)   # validated only: no option changes the robust kernels
        nb = int(self._s.n_opt)
        return self._read_solve(lambda *out: self._call("debug_solve", ctypes.byref(o), ctypes.c_double(lambda_), *out),
                                nb, 4 + nb)

    def shard(self):
        """(caller indices of the landmarks this rank owns, number of its visual edges)."""
        n_p, n_e = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(self._lib.omv_lba_shard(self._h, ctypes.byref(n_p), ctypes.byref(n_e), None), "omv_lba_shard")
        idx = np.zeros(n_p.value, np.int32)
        _lib.check(self._lib.omv_lba_shard(self._h, None, None, _lib.ptr(idx)), "omv_lba_shard")
        return idx, n_e.value

    def set_driver(self, host_driven):
        """True: g2o's LM decisions on the host (read-back per trial); False (default): on the device."""
        _lib.check(self._lib.omv_lba_set_driver(self._h, int(bool(host_driven))), "omv_lba_set_driver")
        return self

    def host_syncs(self):
        """(host waits of the last optimize()'s LM loop, its trials): the device driver waits once per batch."""
        n, t = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self._lib.omv_lba_host_syncs(self._h, ctypes.byref(n), ctypes.byref(t)), "omv_lba_host_syncs")
        return n.value, t.value


HUBER_MONO = float(np.float32(np.sqrt(5.991)))     # thHuberMono / thHuberStereo are floats (Optimizer.cc:1469-1470)
HUBER_STEREO = float(np.float32(np.sqrt(7.815)))


class LocalBundleAdjustment(_StagedBA):
    """Optimizer::LocalBundleAdjustment's optimisation (src/Optimizer.cc:1357-1785) on the visual kind of the device
    bundle-adjustment solver (omv_vba, openmavis_amd/csrc/lba.hip).  The flattened graph is a problem dict (field list:
    openmavis_amd.synth_vba.make_vba_problem, which is omv_vba_problem's):

        ba = LocalBundleAdjustment(max_kf=80, max_cams=4, max_pts=10000, max_edges=200000)
        ba.set_problem(prob)
        res, state = ba.optimize(10, lambda_init=100.0)      # an inertial map; lambda_init <= 0: computeLambdaInit

    `res`: err / err_end, iterations, trials, lambda_, lambda_init and per-edge chi2 + outlier flags (chi2 > 5.991 /
    7.815 or a non-positive depth); `state`: q_cw, t_cw, pts.  The state stays on the device between calls, so the
    merge overload's two rounds are optimize(5), set_levels(...) and optimize(10, huber_mono=0, huber_stereo=0);
    BundleAdjustment is optimize(nIterations, huber_mono=sqrt(5.99) if bRobust else 0, ...).  No CPU fallback."""

    _PREFIX = "omv_vba"
    STATE = ("q_cw", "t_cw", "pts")

    def __init__(self, max_kf=80, max_cams=4, max_pts=40000, max_edges=400000):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.omv_vba_create(int(max_kf), int(max_cams), int(max_pts), int(max_edges), ctypes.byref(h)),
                   "omv_vba_create")
        self._lib, self._h = lib, h
        self._s = self._keep = None

    def set_problem(self, prob):
        from .synth_vba import as_vba_struct
        s, keep = as_vba_struct(prob, _lib.VbaProblem)
        _lib.check(self._lib.omv_vba_set_problem(self._h, ctypes.byref(s)), "omv_vba_set_problem")
        self._s, self._keep = s, keep
        return self

    def set_levels(self, mono_level=None, stereo_level=None):
        """Per-edge levels in the caller's order (0 active, 1 excluded); None: every edge of that kind active."""
        self._need("set_levels")
        lv = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (mono_level, stereo_level)]
        for a, n in zip(lv, (self._s.n_mono, self._s.n_stereo)):
            if a is not None and a.size != n:
                raise ValueError("LocalBundleAdjustment.set_levels: one level per edge")
        _lib.check(self._lib.omv_vba_set_levels(self._h, _lib.ptr(lv[0]), _lib.ptr(lv[1])), "omv_vba_set_levels")
        return self

    @staticmethod
    def _opts(iterations, lambda_init, max_trials, huber_mono, huber_stereo):
        return _lib.VbaOpts(int(iterations), float(lambda_init), int(max_trials), float(huber_mono), float(huber_stereo))

    def optimize(self, iterations=10, lambda_init=0.0, max_trials=10, huber_mono=HUBER_MONO, huber_stereo=HUBER_STEREO,
                 chi2=True):
        self._need("optimize")
        o = self._opts(iterations, lambda_init, max_trials, huber_mono, huber_stereo)
        E, S = self._s.n_mono, self._s.n_stereo
        c_m, c_s = (np.zeros(E), np.zeros(S)) if chi2 else (None, None)
        o_m, o_s = np.zeros(E, np.uint8), np.zeros(S, np.uint8)
        r = _lib.VbaResult()
        r.mono_chi2, r.stereo_chi2 = _lib.ptr(c_m), _lib.ptr(c_s)
        r.mono_outlier, r.stereo_outlier = _lib.ptr(o_m), _lib.ptr(o_s)
        _lib.check(self._lib.omv_vba_optimize(self._h, ctypes.byref(o), ctypes.byref(self._s), ctypes.byref(r)),
                   "omv_vba_optimize")
        res = dict(err=r.err, err_end=r.err_end, iterations=r.iterations, trials=r.trials, lambda_=r.lambda_,
                   lambda_init=r.lambda_init, mono_chi2=c_m, mono_outlier=o_m, stereo_chi2=c_s, stereo_outlier=o_s)
        return res, {k: self._keep[k].copy() for k in self.STATE}

    def reset(self):
        """The state uploaded by set_problem again (device copy; the levels stay)."""
        _lib.check(self._lib.omv_vba_reset(self._h), "omv_vba_reset")
        return self

    def evaluate(self, huber_mono=HUBER_MONO, huber_stereo=HUBER_STEREO):
        """Errors and Jacobians (JXi = d e / d point, JXj = d e / d pose, (omega, upsilon)) at the device state."""
        self._need("evaluate")
        o = self._opts(0, 0.0, 10, huber_mono, huber_stereo)
        E, S = self._s.n_mono, self._s.n_stereo
        out = dict(mono_err=np.zeros((E, 2)), mono_jxi=np.zeros((E, 2, 3)), mono_jxj=np.zeros((E, 2, 6)),
                   stereo_err=np.zeros((S, 3)), stereo_jxi=np.zeros((S, 3, 3)), stereo_jxj=np.zeros((S, 3, 6)))
        _lib.check(self._lib.omv_vba_evaluate(self._h, ctypes.byref(o), *[_lib.ptr(v) for v in out.values()]),
                   "omv_vba_evaluate")
        return out

    def debug_solve(self, lambda_, huber_mono=HUBER_MONO, huber_stereo=HUBER_STEREO):
        """One reduced-system solve at the device state (omv_vba_debug_solve): as LocalInertialBA.debug_solve."""
        self._need("debug_solve")
        o = self._opts(1, 0.0, 10, huber_mono, huber_stereo)
        nb = int(self._s.n_opt)
        return self._read_solve(lambda *out: self._call("debug_solve", ctypes.byref(o), ctypes.c_double(lambda_), *out),
                                nb, 4 + nb)


class FullInertialBA(_StagedBA):
    """Optimizer::FullInertialBA's optimisation (src/Optimizer.cc:368-853) on the full inertial kind of the device
    bundle-adjustment solver (omv_fiba, openmavis_amd/csrc/lba.hip): the whole map, every EdgeInertial Huber at its
    full information, no outlier round.  The flattened map is a problem dict (openmavis_amd.synth_fiba.make_fiba_problem:
    omv_lba_problem's fields plus shared_bias, prior_g, prior_a, bg0, ba0):

        ba = FullInertialBA(max_kf=200, max_cams=5, max_pts=40000, max_edges=400000, max_imu=200)
        ba.set_problem(prob)                       # shared_bias=1: bInit, one bias pair under the two priors
        res, state = ba.optimize(iterations=100)   # lambda_init 1e-5 (:393)

    `res`: err / err_end, iterations, trials, lambda_ and the per-edge chi2 (0 on an edge of a map point that only fixed
    keyframes see: it is no vertex); `state`: Rwb, twb, Rcw, tcw, vel, bg, ba, pts -- with shared_bias every bImu keyframe
    holds the pair.  The state stays on the device between calls.  One rank; no CPU fallback."""

    _PREFIX = "omv_fiba"

    def __init__(self, max_kf=200, max_cams=5, max_pts=40000, max_edges=400000, max_imu=200):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.omv_fiba_create(int(max_kf), int(max_cams), int(max_pts), int(max_edges), int(max_imu),
                                       ctypes.byref(h)), "omv_fiba_create")
        self._lib, self._h = lib, h
        self._s = self._keep = None

    def set_problem(self, prob):
        from .synth_fiba import as_fiba_struct
        s, keep = as_fiba_struct(prob, _lib.FibaProblem, _lib.LbaProblem)
        _lib.check(self._lib.omv_fiba_set_problem(self._h, ctypes.byref(s)), "omv_fiba_set_problem")
        self._s, self._keep = s, keep
        return self

    def optimize(self, iterations=100, lambda_init=1e-5, max_trials=10, chi2=True):
        self._need("optimize")
        o = _lib.FibaOpts(int(iterations), float(lambda_init), int(max_trials))
        E, S = self._s.base.n_mono, self._s.base.n_stereo
        c_m, c_s = (np.zeros(E), np.zeros(S)) if chi2 else (None, None)
        r = _lib.FibaResult()
        r.mono_chi2, r.stereo_chi2 = _lib.ptr(c_m), _lib.ptr(c_s)
        _lib.check(self._lib.omv_fiba_optimize(self._h, ctypes.byref(o), ctypes.byref(self._s), ctypes.byref(r)),
                   "omv_fiba_optimize")
        res = dict(err=r.err, err_end=r.err_end, iterations=r.iterations, trials=r.trials, lambda_=r.lambda_,
                   mono_chi2=c_m, stereo_chi2=c_s)
        return res, read_state(self._keep)

    def reset(self):
        """The state uploaded by set_problem again (device copy)."""
        self._need("reset")
        _lib.check(self._lib.omv_fiba_reset(self._h), "omv_fiba_reset")
        return self

    def evaluate(self):
        """Residuals and visual Jacobians at the device state, in the caller's edge order; prior_err: the two prior
        edges' errors 0 - b (gyro, acc)."""
        self._need("evaluate")
        E, S, I = self._s.base.n_mono, self._s.base.n_stereo, self._s.base.n_imu
        out = dict(mono_err=np.zeros((E, 2)), mono_jx=np.zeros((E, 6)), mono_jp=np.zeros((E, 12)), imu_err=np.zeros((I, 9)),
                   stereo_err=np.zeros((S, 3)), stereo_jx=np.zeros((S, 9)), stereo_jp=np.zeros((S, 18)),
                   prior_err=np.zeros(6))
        _lib.check(self._lib.omv_fiba_evaluate(self._h, *[_lib.ptr(v) for v in out.values()]), "omv_fiba_evaluate")
        return out

    def debug_solve(self, lambda_):
        """One reduced-system solve at the device state (omv_fiba_debug_solve): as LocalInertialBA.debug_solve, with
        n = 16 (n_opt + shared_bias): the shared pair is the last block, rows 9..14 of it."""
        self._need("debug_solve")
        nb = int(self._s.base.n_opt) + int(self._s.shared_bias != 0)
        return self._read_solve(lambda *out: self._call("debug_solve", ctypes.c_double(lambda_), *out), nb, 4 + nb)


class PoseInertialOptimizer:
    """Host-side mirror of Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:5021-5578)
    for a batch of frames on the device (openmavis_amd/csrc/pose.hip).

        opt = PoseInertialOptimizer(max_frames=256, max_edges=400000)
        n_good = opt.PoseInertialOptimizationLastKeyFrame(batch, arrays, kp_outlier, H, bRecInit=False)

    `batch` carries the rig (host numpy: cam, Rcb, tcb, Rbc, tbc, bf, n_frames, n_cams, kp_cap and the
    edge arrays' lengths); `arrays` maps every omv_pose_batch pointer field (state in/out, the last
    keyframe's fixed vertices, preintegration, frame-major edges) to a device tensor.  kp_outlier
    (uint8 [F][kp_cap]) receives Frame::mvbOutlier, H (float64 [F][225] or None) the ConstraintPoseImu
    Hessian; the int32 [F] return tensor holds the reference's return value per frame.  No CPU fallback.
    """

    def __init__(self, max_frames=256, max_edges=400000):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.omv_pose_create(int(max_frames), int(max_edges), ctypes.byref(h)), "omv_pose_create")
        self._lib, self._h = lib, h

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.omv_pose_destroy(self._h)
            self._h = None

    AUTO, BATCH, GROUPED = 0, 1, 2

    def set_mode(self, mode, parts=0):
        """Kernel choice (omv_pose_set_mode): AUTO (grouped kernel up to 16 frames per call, else one workgroup per
        frame), BATCH or GROUPED (`parts` workgroups per frame; 0 = one per 126 (LastFrame) / 190 (LastKeyFrame)
        visual edges of the mean frame, at least ceil(batch edges / 1022), at most 48 -- include/omv.h)."""
        _lib.check(self._lib.omv_pose_set_mode(self._h, int(mode), int(parts)), "omv_pose_set_mode")
        return self

    def last_error(self, stream=None):
        """Device error word since the last read (0, or OMV_ERR_CAPACITY / OMV_ERR_HIP from the grouped kernel)."""
        import torch
        e = ctypes.c_int32(0)
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(self._lib.omv_pose_last_error(self._h, ctypes.byref(e), ctypes.c_void_p(st)), "omv_pose_last_error")
        return e.value

    EDGE_KEYS = ("mono_start", "mono_cam", "mono_kp", "mono_obs", "mono_inv_sigma2", "mono_xw", "mono_close",
                 "stereo_start", "stereo_cam", "stereo_kp", "stereo_obs", "stereo_inv_sigma2", "stereo_xw")

    @staticmethod
    def edge_arrays(max_edges, device):
        """Device buffers for one frame's edge lists (the omv_pose_batch edge fields of a one-frame batch)."""
        import torch
        z = dict(device=device)
        E = int(max_edges)
        return dict(mono_start=torch.zeros(2, dtype=torch.int32, **z), mono_cam=torch.zeros(E, dtype=torch.int32, **z),
                    mono_kp=torch.zeros(E, dtype=torch.int32, **z), mono_obs=torch.zeros((E, 2), dtype=torch.float64, **z),
                    mono_inv_sigma2=torch.zeros(E, dtype=torch.float32, **z),
                    mono_xw=torch.zeros((E, 3), dtype=torch.float32, **z), mono_close=torch.zeros(E, dtype=torch.uint8, **z),
                    stereo_start=torch.zeros(2, dtype=torch.int32, **z),
                    stereo_cam=torch.zeros(E, dtype=torch.int32, **z), stereo_kp=torch.zeros(E, dtype=torch.int32, **z),
                    stereo_obs=torch.zeros((E, 3), dtype=torch.float64, **z),
                    stereo_inv_sigma2=torch.zeros(E, dtype=torch.float32, **z),
                    stereo_xw=torch.zeros((E, 3), dtype=torch.float32, **z))

    def EdgesFromMatches(self, kps, n_kp, kp_to_mp, mp_pos, mp_track_depth, inv_level_sigma2, arrays, uright=None,
                         stream=None):
        """The edge-creation loop of PoseInertialOptimizationLastKeyFrame / LastFrame (src/Optimizer.cc:5079-5330)
        for ONE multi-camera frame, on the device (omv_pose_edges_from_matches): kps int32 [C][kp_cap][6] (omv_kp
        rows), n_kp [C], kp_to_mp [C*kp_cap] (SearchByProjection's assignment), mp_pos float [M][3], mp_track_depth
        [M], inv_level_sigma2 host sequence (Frame::mvInvLevelSigma2), uright float [C][kp_cap] or None; writes the
        edge lists into `arrays` (edge_arrays' buffers; their length bounds the edge count).  Asynchronous."""
        import torch
        C, cap = int(kps.shape[-3]), int(kps.shape[-2])
        E = int(arrays["mono_cam"].shape[0])
        lv = (ctypes.c_float * 16)(*[float(x) for x in inv_level_sigma2][:16])
        st = stream if stream is not None else torch.cuda.current_stream(kps.device).cuda_stream
        a = arrays
        _lib.check(self._lib.omv_pose_edges_from_matches(
            self._h, C, cap, _lib.ptr(kps), _lib.ptr(n_kp), _lib.ptr(kp_to_mp), _lib.ptr(mp_pos),
            _lib.ptr(mp_track_depth), lv, len(inv_level_sigma2), _lib.ptr(uright), E,
            *[_lib.ptr(a[k]) for k in self.EDGE_KEYS], ctypes.c_void_p(st)), "omv_pose_edges_from_matches")
        return arrays

    def PoseInertialOptimizationLastKeyFrame(self, batch, arrays, kp_outlier, H=None, bRecInit=False, stream=None):
        import torch
        from .synth_pose import as_pose_struct
        s, keep = as_pose_struct(batch, _lib.PoseBatch, arrays)
        n_good = torch.zeros(s.n_frames, dtype=torch.int32, device=kp_outlier.device)
        st = stream if stream is not None else torch.cuda.current_stream(kp_outlier.device).cuda_stream
        _lib.check(self._lib.omv_pose_inertial_last_kf(self._h, ctypes.byref(s), int(bool(bRecInit)),
                                                       _lib.ptr(kp_outlier), _lib.ptr(n_good), _lib.ptr(H),
                                                       ctypes.c_void_p(st)),
                   "omv_pose_inertial_last_kf")
        del keep
        return n_good

    def PoseInertialOptimizationLastFrame(self, batch, arrays, kp_outlier, H=None, bRecInit=False, stream=None):
        """Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:5580-6170) on every frame of the
        batch.  As PoseInertialOptimizationLastKeyFrame, but `arrays`' kf_* tensors hold the previous
        frame's vertices (free here, not written back), `preint` is mpImuPreintegratedFrame, and `arrays`
        also carries the previous frame's ConstraintPoseImu (prior_Rwb / prior_twb / prior_vel / prior_bg /
        prior_ba, prior_H [F][225]) and preint_kf (mpImuPreintegrated).  H receives Marginalize's frame
        block; ConstraintPoseImu() turns it into the next prior."""
        import torch
        from .synth_pose import as_pose_struct, as_prior_struct
        s, keep = as_pose_struct(batch, _lib.PoseBatch, arrays)
        pr = as_prior_struct(_lib.PosePrior, arrays)
        n_good = torch.zeros(s.n_frames, dtype=torch.int32, device=kp_outlier.device)
        st = stream if stream is not None else torch.cuda.current_stream(kp_outlier.device).cuda_stream
        _lib.check(self._lib.omv_pose_inertial_last_frame(self._h, ctypes.byref(s), ctypes.byref(pr),
                                                          int(bool(bRecInit)), _lib.ptr(kp_outlier), _lib.ptr(n_good),
                                                          _lib.ptr(H), ctypes.c_void_p(st)),
                   "omv_pose_inertial_last_frame")
        del keep
        return n_good

    def PoseOptimization(self, batch, arrays, pose_q, pose_t, kp_outlier, stream=None):
        """Optimizer::PoseOptimization (src/Optimizer.cc:855-1278) on every frame of the batch (omv_pose_optimization):
        `batch` as above plus rig_q / rig_t (host [n_cams][4] / [3], T_c0 = mTrl / mTsll / mTsrl); `arrays` needs only
        the edge tensors (EDGE_KEYS); pose_q / pose_t (float64 device [F][4] (x y z w) / [F][3]) hold Frame::GetPose()
        and receive the optimised Tcw; kp_outlier (uint8 [F][kp_cap]) receives mvbOutlier.  Returns the int32 [F]
        return values (nInitialCorrespondences - nBad).  Asynchronous; no CPU fallback."""
        import numpy as np
        import torch
        from .synth_pose import as_pose_struct
        s, keep = as_pose_struct(batch, _lib.PoseBatch, arrays)
        rq = np.ascontiguousarray(batch["rig_q"], np.float64)
        rt = np.ascontiguousarray(batch["rig_t"], np.float64)
        n_good = torch.zeros(s.n_frames, dtype=torch.int32, device=kp_outlier.device)
        st = stream if stream is not None else torch.cuda.current_stream(kp_outlier.device).cuda_stream
        _lib.check(self._lib.omv_pose_optimization(self._h, ctypes.byref(s), _lib.ptr(rq), _lib.ptr(rt), _lib.ptr(pose_q),
                                                   _lib.ptr(pose_t), _lib.ptr(kp_outlier), _lib.ptr(n_good),
                                                   ctypes.c_void_p(st)), "omv_pose_optimization")
        del keep
        return n_good

    @staticmethod
    def ConstraintPoseImu(H, out=None, stream=None):
        """The ConstraintPoseImu ctor's projection (include/G2oTypes.h:639-659) of device float64 [n][225]
        matrices; returns `out` (may be H itself)."""
        import torch
        lib = _lib.load()
        out = torch.empty_like(H) if out is None else out
        st = stream if stream is not None else torch.cuda.current_stream(H.device).cuda_stream
        _lib.check(lib.omv_pose_constraint(int(H.shape[0]), _lib.ptr(H), _lib.ptr(out), ctypes.c_void_p(st)),
                   "omv_pose_constraint")
        return out


# ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:2460-2726) -------------------------------------------------------------
OPTSIM3_KEPT, OPTSIM3_INLIER, OPTSIM3_REMOVED_1, OPTSIM3_REMOVED_2 = 0, 1, 2, 3


def select_sim3_edges(matched, cam_of_kp1, cameraID1, mp1_ok, mp2_ok, i2, bAllPoints=False):
    """The graph-side filter of OptimizeSim3's loop over vpMatches1 (:2522-2589) on arrays of length N =
    vpMatches1.size(): matched[i] = vpMatches1[i] != NULL; cam_of_kp1[i] = pKF1->kpIdxToCamIdx(i); mp1_ok[i] =
    vpMapPoints1[i] && !isBad(); mp2_ok[i] = !vpMatches1[i]->isBad(); i2[i] = the index of vpMatches1[i] in pKF2 on
    cameraID2 (-1: not seen there).  Returns (index1, has_kp2): the i that become entries of a job, ascending, and whether
    each has a KF2 keypoint.  The P3D2c.z < 0 test needs the geometry and is the kernel's."""
    matched, mp1_ok, mp2_ok = (np.asarray(a, bool).reshape(-1) for a in (matched, mp1_ok, mp2_ok))
    i2 = np.asarray(i2, np.int64).reshape(-1)
    keep = matched & (np.asarray(cam_of_kp1, np.int64).reshape(-1) == int(cameraID1)) & mp1_ok & mp2_ok
    keep &= (i2 >= 0) | bool(bAllPoints)
    idx = np.nonzero(keep)[0].astype(np.int32)
    return idx, i2[idx] >= 0


class Sim3Optimizer:
    """One omv_optsim3 handle (openmavis_amd/csrc/optsim3.hip): OptimizeSim3 for up to max_jobs candidate pairs and
    max_entries correspondences per call.  A job is a dict: per entry index1 [N], Xw1, Xw2 [N][3], obs1 [N][2],
    inv_sigma2_1 [N], has_kp2 [N], obs2 [N][2], inv_sigma2_2 [N]; per job pose1, pose2 [12] (Riw row-major, tiw), cam1,
    cam2 [8], model1, model2 (_lib.CAM_KB8 / CAM_PINHOLE), fix_scale, th2 and g2oS12 as q [4] (x y z w), t [3], s.
    There is no CPU fallback."""

    _ENTRY = (("Xw1", np.float32, 3), ("Xw2", np.float32, 3), ("obs1", np.float32, 2), ("inv_sigma2_1", np.float32, 1),
              ("has_kp2", np.uint8, 1), ("obs2", np.float32, 2), ("inv_sigma2_2", np.float32, 1))
    _JOB = (("pose1", np.float32, 12), ("pose2", np.float32, 12), ("cam1", np.float32, 8), ("cam2", np.float32, 8),
            ("model1", np.int32, 1), ("model2", np.int32, 1), ("fix_scale", np.int32, 1), ("th2", np.float32, 1))

    def __init__(self, max_jobs=8, max_entries=4096, stream=None):
        self._lib, self.stream = _lib.load(), stream
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.omv_optimize_sim3_create(int(max_jobs), int(max_entries), ctypes.byref(self._h)),
                   "omv_optimize_sim3_create")
        self.n = np.zeros(0, np.int32)

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.omv_optimize_sim3_destroy(self._h)
            self._h = ctypes.c_void_p()

    def _stream(self):
        if self.stream is not None:
            return ctypes.c_void_p(self.stream.cuda_stream)
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(self, jobs):
        """omv_optimize_sim3 on `jobs`; returns (status code, n_in [J], q [J][4], t [J][3], s [J], status per job)."""
        J = len(jobs)
        n = np.array([len(np.asarray(j["Xw1"]).reshape(-1, 3)) for j in jobs], np.int32)
        start = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)

        def cat(key, dt, width):
            if not J:
                return np.zeros((0, width), dt)
            return np.ascontiguousarray(np.concatenate([np.asarray(j[key], dt).reshape(-1, width) for j in jobs]))

        entry = [cat(k, dt, w) for k, dt, w in self._ENTRY]
        per_job = [cat(k, dt, w) for k, dt, w in self._JOB]
        q, t, s = cat("q", np.float64, 4), cat("t", np.float64, 3), cat("s", np.float64, 1)
        n_in = np.zeros(max(J, 1), np.int32)
        status = np.zeros(max(int(start[-1]), 1), np.uint8)
        code = self._lib.omv_optimize_sim3(self._h, J, _lib.ptr(start), *[_lib.ptr(a) for a in entry + per_job],
                                           _lib.ptr(q), _lib.ptr(t), _lib.ptr(s), _lib.ptr(n_in), _lib.ptr(status),
                                           self._stream())
        if code == _lib.OMV_OK:
            self.n = n
        return code, n_in[:J], q, t, s.reshape(-1), [status[start[j]:start[j + 1]] for j in range(J)]

    def debug(self, j):
        """The library's test hook for job j of the last run: dict(H [7][7], b, chi2, lambda_init, x, e12, e21 [N][2],
        iterations, trials, max_trials [2])."""
        N = int(self.n[j])
        o = dict(H=np.zeros((7, 7)), b=np.zeros(7), chi2=np.zeros(1), lambda_init=np.zeros(1), x=np.zeros(7),
                 e12=np.zeros((max(N, 1), 2)), e21=np.zeros((max(N, 1), 2)), iterations=np.zeros(2, np.int32),
                 trials=np.zeros(2, np.int32), max_trials=np.zeros(2, np.int32))
        _lib.check(self._lib.omv_optimize_sim3_debug(self._h, int(j), *[_lib.ptr(v) for v in o.values()], self._stream()),
                   "omv_optimize_sim3_debug")
        o["chi2"], o["lambda_init"] = float(o["chi2"][0]), float(o["lambda_init"][0])
        o["e12"], o["e21"] = o["e12"][:N], o["e21"][:N]
        return o


def OptimizeSim3(jobs, vpMatches1=None, optimizer=None):
    """Optimizer::OptimizeSim3 for every job of `jobs` in one device call.  Returns per job (nIn, g2oS12, matches):
    g2oS12 = dict(q, t, s) -- the input where the reference returns 0 before writing it back -- and matches, the
    surviving part of vpMatches1: vpMatches1[j] (one bool array of length vpMatches1.size() per job; default: true at
    the job's index1 in an array just long enough) with the entries the reference nulls set false.  mAcumHessian is
    the zero 7 x 7 the reference leaves and is not returned.  `optimizer`: a Sim3Optimizer to reuse."""
    jobs = list(jobs)
    n_entries = sum(len(np.asarray(j["Xw1"]).reshape(-1, 3)) for j in jobs)
    opt = optimizer if optimizer is not None else Sim3Optimizer(max(len(jobs), 1), n_entries)
    code, n_in, q, t, s, status = opt.run(jobs)
    _lib.check(code, "omv_optimize_sim3")
    out = []
    for j, job in enumerate(jobs):
        idx = np.asarray(job["index1"], np.int64).reshape(-1)
        if vpMatches1 is not None:
            m = np.array(vpMatches1[j], bool)
        else:
            m = np.zeros(int(idx.max()) + 1 if len(idx) else 0, bool)
            m[idx] = True
        m[idx[status[j] >= OPTSIM3_REMOVED_1]] = False
        out.append((int(n_in[j]), dict(q=q[j].copy(), t=t[j].copy(), s=float(s[j])), m))
    return out


class EssentialGraph(_BlockSolverHandle):
    """The pose graphs of loop closing and map merging (Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:1826-2119, its
    merge overload :2121-2458, and OptimizeEssentialGraph4DoF :6171-6480) on the device (omv_essgraph,
    openmavis_amd/csrc/essgraph.hip): g2o's Levenberg-Marquardt with the edges' numeric Jacobians on the block LDL^T of
    the bundle-adjustment solver.  The flattened graph is a problem dict (openmavis_amd.synth_essgraph):

        g = EssentialGraph("sim3", max_vertices=2000, max_edges=20000)        # or "4dof"
        g.set_problem(prob)            # vertices, fixed, S_a, S_b, edge_i, edge_j, edge_table, fix_scale [, Rcb, tcb]
        res = g.optimize(iterations=20, max_trials=10)
        poses, points = g.recover("loop", prob["points"], prob["point_ref"])

    `res`: err / err_end, iterations, trials, solver_failed, lambda_ and the final vertices.  The state stays on the
    device between calls.  One rank; no CPU fallback."""

    _PREFIX = "omv_essgraph"
    KINDS = {"sim3": _lib.ESSGRAPH_SIM3, "4dof": _lib.ESSGRAPH_4DOF}
    MODES = {"loop": _lib.ESSGRAPH_RECOVER_LOOP, "merge": _lib.ESSGRAPH_RECOVER_MERGE, "4dof": _lib.ESSGRAPH_RECOVER_4DOF}

    def __init__(self, kind="sim3", max_vertices=2000, max_edges=20000):
        lib = _lib.load()
        h = ctypes.c_void_p()
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        _lib.check(lib.omv_essgraph_create(self.kind, int(max_vertices), int(max_edges), ctypes.byref(h)),
                   "omv_essgraph_create")
        self._lib, self._h = lib, h
        self._s = self._keep = None

    @property
    def _sim3(self):
        return self.kind == _lib.ESSGRAPH_SIM3

    def set_problem(self, prob):
        s, keep = essgraph_struct(prob)
        _lib.check(self._lib.omv_essgraph_set_problem(self._h, ctypes.byref(s)), "omv_essgraph_set_problem")
        self._s, self._keep = s, keep
        return self

    def optimize(self, iterations=20, max_trials=10):
        self._need("optimize")
        v = np.zeros((self._s.n_vertices, 8 if self._sim3 else 24))
        r = _lib.EssGraphResult()
        r.vertices = _lib.ptr(v)
        _lib.check(self._lib.omv_essgraph_optimize(self._h, int(iterations), int(max_trials), ctypes.byref(r)),
                   "omv_essgraph_optimize")
        return dict(err=r.err, err_end=r.err_end, iterations=r.iterations, trials=r.trials,
                    solver_failed=r.solver_failed, lambda_=r.lambda_, vertices=v)

    def evaluate(self):
        """Per edge at the device state: err, g2o's numeric jac_i / jac_j (rows x variables), the composed measurement
        and chi2."""
        self._need("evaluate")
        E = self._s.n_edges
        D, V, M = (7, 7, 8) if self._sim3 else (6, 4, 12)
        out = dict(err=np.zeros((E, D)), jac_i=np.zeros((E, D, V)), jac_j=np.zeros((E, D, V)), meas=np.zeros((E, M)),
                   chi2=np.zeros(E))
        _lib.check(self._lib.omv_essgraph_evaluate(self._h, *[_lib.ptr(v) for v in out.values()]), "omv_essgraph_evaluate")
        return out

    def reset(self):
        """The state uploaded by set_problem again (device copy)."""
        self._need("reset")
        _lib.check(self._lib.omv_essgraph_reset(self._h), "omv_essgraph_reset")
        return self

    def debug_solve(self, lambda_):
        """One linear solve at the device state (omv_essgraph_debug_solve): the n x n system, rhs, x, the failure flag
        and the plan (storage mode, stored blocks, blocks in LDS, levels, columns per level)."""
        self._need("debug_solve")
        nb, nl = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self._lib.omv_essgraph_blocks(self._h, ctypes.byref(nb), ctypes.byref(nl)), "omv_essgraph_blocks")
        return self._read_solve(lambda *out: self._call("debug_solve", ctypes.c_double(lambda_), *out), nb.value,
                                4 + nl.value)

    def recover(self, mode, points=None, point_ref=None):
        """The epilogue: the SE3f of every keyframe's SetPose as [n][7] (unit quaternion x y z w, translation) and the
        corrected map points (a copy; point_ref -1 leaves a point as it was)."""
        self._need("recover")
        m = self.MODES[mode] if isinstance(mode, str) else int(mode)
        poses = np.zeros((self._s.n_vertices, 7), np.float32)
        pts = np.ascontiguousarray(points, np.float32).copy() if points is not None else np.zeros((0, 3), np.float32)
        ref = np.ascontiguousarray(point_ref, np.int32) if point_ref is not None else np.zeros(0, np.int32)
        _lib.check(self._lib.omv_essgraph_recover(self._h, m, _lib.ptr(poses), len(pts), _lib.ptr(pts), _lib.ptr(ref)),
                   "omv_essgraph_recover")
        return poses, pts

    def last_ms(self):
        ms = ctypes.c_double(0)
        _lib.check(self._lib.omv_essgraph_last_ms(self._h, ctypes.byref(ms)), "omv_essgraph_last_ms")
        return ms.value


def essgraph_struct(prob):
    """A problem dict as omv_essgraph_problem and the arrays it points into."""
    keep = dict(vertices=np.ascontiguousarray(prob["vertices"], np.float64),
                fixed=np.ascontiguousarray(prob["fixed"], np.uint8),
                S_a=np.ascontiguousarray(prob["S_a"], np.float64), S_b=np.ascontiguousarray(prob["S_b"], np.float64),
                edge_i=np.ascontiguousarray(prob["edge_i"], np.int32), edge_j=np.ascontiguousarray(prob["edge_j"], np.int32),
                edge_table=np.ascontiguousarray(prob["edge_table"], np.int32))
    for k in ("Rcb", "tcb"):
        keep[k] = np.ascontiguousarray(prob[k], np.float64) if prob.get(k) is not None else None
    s = _lib.EssGraphProblem()
    s.n_vertices, s.n_edges, s.fix_scale = len(keep["vertices"]), len(keep["edge_i"]), int(prob.get("fix_scale", 0))
    for k, v in keep.items():
        setattr(s, k, _lib.ptr(v))
    return s, keep


def _optimize_essential_graph(kind, mode, prob, iterations, max_trials, handle):
    g = handle or EssentialGraph(kind, max_vertices=len(prob["vertices"]), max_edges=max(len(prob["edge_i"]), 1))
    res = g.set_problem(prob).optimize(iterations, max_trials)
    poses, points = g.recover(mode, prob.get("points"), prob.get("point_ref"))
    return dict(res, poses=poses, points=points)


def OptimizeEssentialGraph(prob, iterations=20, max_trials=10, merge=False, handle=None):
    """Optimizer::OptimizeEssentialGraph on a flat problem dict: optimize(20) and the epilogue (SetPose's SE3f per
    keyframe, the corrected map points).  merge: the map-merging overload's pose recovery (t / s in double)."""
    return _optimize_essential_graph("sim3", "merge" if merge else "loop", prob, iterations, max_trials, handle)


def OptimizeEssentialGraph4DoF(prob, iterations=20, max_trials=10, handle=None):
    """Optimizer::OptimizeEssentialGraph4DoF on a flat problem dict (vertices [Rcw | tcw | Rwb | twb], Rcb, tcb)."""
    return _optimize_essential_graph("4dof", "4dof", prob, iterations, max_trials, handle)
