"""dvo::core::PointSelection and dvo::DenseTracker: the alignment calls themselves."""
import ctypes as C

import numpy as np

from . import _lib
from .context import default_context
from .api_types import Config, Result, _RESULT_DTYPE, _unpack_stats
from .planes import FrameSet, _fp, _handles


class PointSelection:
    """Reference-side selection cache (point_selection.h:69-99).  The selected list itself never leaves the GPU."""

    def __init__(self, pyramid=None, intensity_threshold=0.0, depth_threshold=0.0):
        self.pyramid = pyramid
        self.intensity_threshold, self.depth_threshold = intensity_threshold, depth_threshold

    def setRgbdImagePyramid(self, pyramid):
        self.pyramid = pyramid

    recycle = setRgbdImagePyramid

    def getRgbdImagePyramid(self):
        assert self.pyramid is not None
        return self.pyramid

    def getMaximumNumberOfPoints(self, level):     # point_selection.cpp:68-71
        c = self.pyramid.camera
        return int(c.width * c.height * 0.25 ** level)

    def select(self, level, want_mask=False):
        """Returns the number of selected points (and the uint8 mask if asked): the thresholds' selection combined with the
        pyramid's caller selection (RgbdImagePyramid.set_selection)."""
        p = self.pyramid
        p.build(level + 1)
        n = C.c_int()
        mask = None
        mp = None
        if want_mask:
            img = p.level(level)
            mask = np.zeros((img.height, img.width), np.uint8)
            mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        p.ctx.check(p.ctx._lib.dvo_hip_frame_select(p.ctx.ptr, p.ptr, level, self.intensity_threshold, self.depth_threshold,
                                                   C.byref(n), mp))
        return (n.value, mask) if want_mask else n.value


class DenseTracker:
    """dvo::DenseTracker (dense_tracking.h:142-162).  Not re-entrant, like the reference: one per thread."""
    _default_config = Config()

    @staticmethod
    def getDefaultConfig():
        return DenseTracker._default_config

    def __init__(self, config=None, ctx=None):
        self.ctx = ctx or default_context()
        self.reference_selection_ = PointSelection()
        self.configure(config or DenseTracker.getDefaultConfig())

    def configure(self, config):
        assert config.IsSane()                                   # dense_tracking.cpp:74
        self.cfg = Config(**config.__dict__)
        self.reference_selection_.intensity_threshold = config.IntensityDerivativeThreshold
        self.reference_selection_.depth_threshold = config.DepthDerivativeThreshold

    def configuration(self):
        return self.cfg

    def match(self, reference, current, result_or_transformation, with_stats=True):
        """match(RgbdImagePyramid|PointSelection reference, RgbdImagePyramid current, Result& | 4x4 ndarray (in/out)).
        Always returns True; failure shows as Result.isNaN() / termination criteria."""
        ref_pyr = reference.getRgbdImagePyramid() if isinstance(reference, PointSelection) else reference
        if isinstance(result_or_transformation, Result):
            self.match_batch([ref_pyr], [current], [result_or_transformation], with_stats=with_stats)
            return True
        T = result_or_transformation
        r = Result()
        r.Transformation = np.array(T, dtype=np.float64)
        self.match_batch([ref_pyr], [current], [r], with_stats=False)
        T[...] = r.Transformation
        return True

    def match_batch(self, references, currents, results, with_stats=False):
        """n independent alignments in one batched launch sequence (keyframe_graph.cpp:576-593 shape)."""
        n = len(references)
        assert len(currents) == n and len(results) == n
        cfg = self.cfg
        for r, c in zip(references, currents):
            r.build(cfg.getNumLevels())                           # dense_tracking.cpp:125, 133
            c.build(cfg.getNumLevels())
        cres = (_lib.Result * n)()
        for i, r in enumerate(results):
            if cfg.UseInitialEstimate:
                assert not r.isNaN(), "Provided initialization is NaN!"   # dense_tracking.cpp:139
            else:
                r.setIdentity()
            for k, v in enumerate(np.asarray(r.Transformation, dtype=np.float64).reshape(-1)):
                cres[i].transformation[k] = v
        refs, curs = _handles(references), _handles(currents)
        ccfg = cfg.to_c()
        nl = cfg.FirstLevel - cfg.LastLevel + 1
        cap_it = nl * cfg.MaxIterationsPerLevel
        if with_stats:
            levels = (_lib.LevelStats * (n * nl))()
            iters = (_lib.IterationStats * (n * cap_it))()
            rc = self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, levels, nl, iters, cap_it)
        else:
            rc = self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, None, 0, None, 0)
        self.ctx.check(rc)
        for i, r in enumerate(results):
            r.Transformation = np.array(cres[i].transformation).reshape(4, 4)
            r.Information = np.array(cres[i].information).reshape(6, 6)
            r.LogLikelihood = cres[i].loglik
            # keyframe-selection statistics computed on the device (extension over the reference's Result)
            r.Entropy, r.ConditionNumber = cres[i].entropy, cres[i].condition_number
            r.ConstraintRatio, r.ConstraintRatioAccepted = cres[i].constraint_ratio, cres[i].constraint_ratio_accepted
            if with_stats:   # appended, not cleared
                r.Statistics.Levels.extend(_unpack_stats(cres[i], levels[i * nl:(i + 1) * nl], iters[i * cap_it:(i + 1) * cap_it]))
        return True

    def match_batch_arrays(self, references, currents, T_init=None):
        """match_batch without per-pair Python objects: returns dict(T [n,4,4], information [n,6,6], loglik [n],
        n_iterations [n]).  T_init: optional [n,4,4] initial guesses (used when UseInitialEstimate)."""
        n = len(references)
        cfg = self.cfg
        if not (isinstance(references, FrameSet) and isinstance(currents, FrameSet)):   # a FrameSet's pyramids are final
            for r, c in zip(references, currents):
                r.build(cfg.getNumLevels())
                c.build(cfg.getNumLevels())
        cres = (_lib.Result * n)()
        view = np.frombuffer(cres, dtype=_RESULT_DTYPE)
        if cfg.UseInitialEstimate:
            assert T_init is not None and np.isfinite(T_init).all(), "Provided initialization is NaN!"
            view["transformation"][:] = np.asarray(T_init, dtype=np.float64).reshape(n, 16)
        else:
            view["transformation"][:] = np.eye(4).reshape(16)
        refs, curs = _handles(references), _handles(currents)
        ccfg = cfg.to_c()
        self.ctx.check(self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, None, 0, None, 0))
        return dict(T=view["transformation"].reshape(n, 4, 4).copy(), information=view["information"].reshape(n, 6, 6).copy(),
                    loglik=view["loglik"].copy(), n_iterations=view["n_iterations_total"].copy(), entropy=view["entropy"].copy(),
                    condition_number=view["condition_number"].copy(), constraint_ratio=view["constraint_ratio"].copy(),
                    constraint_ratio_accepted=view["constraint_ratio_accepted"].copy())

    def level_iteration(self, reference, current, level, T34, P_prev=None, first=True, want_residuals=False):
        """One Gauss-Newton linearisation at a fixed estimate (parity entry point, dvo_hip_level_iteration)."""
        T34 = np.ascontiguousarray(np.asarray(T34, dtype=np.float32).reshape(-1)[:12])
        Pp = np.zeros(4, np.float32) if P_prev is None else np.ascontiguousarray(np.asarray(P_prev, np.float32).reshape(-1))
        out = _lib.IterationOut()
        img = current.level(level)
        res = np.empty((img.height, img.width, 2), np.float32) if want_residuals else None
        self.ctx.check(self.ctx._lib.dvo_hip_level_iteration(
            self.ctx.ptr, reference.ptr, current.ptr, level, self.cfg.IntensityDerivativeThreshold, self.cfg.DepthDerivativeThreshold,
            _fp(T34), _fp(Pp), int(first), C.byref(out), _fp(res) if want_residuals else None))
        d = dict(n=out.n, n_selected=out.n_selected, cov=np.array(out.scale_cov), P=np.array(out.precision).reshape(2, 2),
                 neg_ll=out.neg_loglik, A=np.array(out.A).reshape(6, 6), b=np.array(out.b))
        if want_residuals:
            d["residuals"] = res
        return d

    def time_residual_kernel(self, references, currents, level, reps=20, warm_iterations=3):
        """Average duration (ms) of one launch of the fused residual/Jacobian/reduce/log-likelihood kernel (HIP events), after
        `warm_iterations` Gauss-Newton steps on that level (converged transform, t-distribution weights on; 0 = identity)."""
        n = len(references)
        refs, curs, ms = _handles(references), _handles(currents), C.c_float()
        self.ctx.check(self.ctx._lib.dvo_hip_time_residual_kernel(self.ctx.ptr, n, refs, curs, level, warm_iterations, reps, C.byref(ms)))
        return ms.value

    def time_stream_mix(self, references, currents, level, reps=20, with_write=False):
        """Average duration (ms) of a kernel that only streams the planes the level's sweep reads (window sweep: 16 B per pixel, gathering
        sweep: 32 B; with_write: + 8 B written)."""
        n = len(references)
        refs, curs, ms = _handles(references), _handles(currents), C.c_float()
        self.ctx.check(self.ctx._lib.dvo_hip_time_stream_mix(self.ctx.ptr, n, refs, curs, level, int(with_write), reps, C.byref(ms)))
        return ms.value
