"""What the calls that read pyramids at one level refuse before anything reaches the library, and in which order (tracker.py:
_map_frames_args, _warp_args, _covis_args, CodebookLogic._frames_arg).  The pyramids are stubs: no library, no GPU.  Every message
below was recorded from the code as it stood before the four checks were put on one helper."""
import numpy as np
import pytest

from dvo_slam_amd import tracker


class Camera:
    def __init__(self, width=32, height=24):
        self.width, self.height = width, height


class Pyramid:
    def __init__(self, ctx, levels=2, camera=None):
        self.ctx, self.levels, self.camera = ctx, levels, camera or Camera()


class Book(tracker.CodebookLogic):
    def _open(self, m, capacity, seed, ferns):
        pass


CTX, OTHER = object(), object()
EYE = np.eye(4)
NAN = np.full((4, 4), np.nan)


def pyramids(n=2, ctx=CTX, levels=2):
    return [Pyramid(ctx, levels) for _ in range(n)]


def map_args(ps, level=0, poses=None, lo=0.0, hi=1.0):
    return tracker._map_frames_args(ps, [EYE] * len(ps) if poses is None else poses, level, lo, hi, "w")


def warp_args(ps, level=0, others=None, transforms=None):
    return tracker._warp_args(ps, others, [EYE] * len(ps) if transforms is None else transforms, level, "w")


def covis_args(ps, level=0, pairs=((0, 1),), transforms=None):
    return tracker._covis_args(ps, pairs, [EYE] * len(pairs) if transforms is None else transforms, level, "w")


def book_args(ps, level=0, limit=None, ctx=CTX):
    return Book(ctx)._frames_arg(ps, level, "w", limit)


CALLERS = [map_args, warp_args, covis_args, book_args]
FOREIGN = {map_args: "w: the pyramids belong to different contexts", warp_args: "w: the pyramids belong to different contexts",
           covis_args: "w: the pyramids belong to different contexts", book_args: "w: a pyramid of another context than the book's"}


def refused(kind, message, call, *args, **kwargs):
    with pytest.raises(kind) as e:
        call(*args, **kwargs)
    assert type(e.value) is kind and str(e.value) == message


@pytest.mark.parametrize("call", CALLERS)
def test_the_shared_refusals(call):
    refused(ValueError, "w: no pyramids", call, [])
    refused(TypeError, "w: level must be an integer", call, pyramids(), level=True)
    refused(TypeError, "w: level must be an integer", call, pyramids(), level=1.0)
    refused(ValueError, "w: a pyramid of 2 levels has no level 2", call, pyramids(), level=2)
    refused(ValueError, "w: a pyramid of 2 levels has no level -1", call, pyramids(), level=-1)
    refused(ValueError, FOREIGN[call], call, pyramids(1) + pyramids(1, OTHER))
    assert call(pyramids(), level=np.int64(1)) is not None


def test_counts_and_poses():
    refused(ValueError, "w: 2 pyramids but 3 poses", map_args, pyramids(), poses=[EYE] * 3)
    refused(ValueError, "w: 2 items but 1 poses", warp_args, pyramids(), transforms=[EYE])
    refused(ValueError, "w: 2 raster pyramids but 1 sampled pyramids", warp_args, pyramids(), others=pyramids(1))
    refused(ValueError, "w: 1 pairs but 2 poses", covis_args, pyramids(), transforms=[EYE] * 2)
    refused(ValueError, "w: 3 pyramids, one call takes 2", book_args, pyramids(3), limit=2)
    # a pose that is not finite: the warps and covisibility refuse it, a map call leaves it to the kernels
    refused(ValueError, "w: a pose has an entry that is not finite", warp_args, pyramids(), transforms=[EYE, NAN])
    refused(ValueError, "w: a pose has an entry that is not finite", covis_args, pyramids(), transforms=[NAN])
    n, T = map_args(pyramids(), poses=[EYE, NAN])
    assert n == 2 and T.shape == (2, 4, 4) and np.isnan(T[1]).all()


def test_what_the_callers_hand_back():
    n, T = map_args(pyramids(3), level=1)
    assert n == 3 and T.dtype == np.float64 and T.shape == (3, 4, 4) and T.flags.c_contiguous
    n, T = warp_args(pyramids(2), others=pyramids(2))
    assert n == 2 and T.shape == (2, 4, 4)
    P, T = covis_args(pyramids(2), pairs=[(0, 1), (1, 1)])
    assert P.dtype == np.int32 and P.tolist() == [[0, 1], [1, 1]] and P.flags.c_contiguous and T.shape == (2, 4, 4)
    ps = pyramids(2)
    assert book_args(tuple(ps), limit=2) == ps
    assert book_args(pyramids(1) + pyramids(1, OTHER), ctx=None) is not None      # a book without a context takes any pyramid


def test_the_order_of_two_refusals():
    mixed = pyramids(1) + pyramids(1, OTHER)
    # the list before everything else
    refused(ValueError, "w: no pyramids", map_args, [], level=True, poses=[EYE])
    refused(ValueError, "w: no pyramids", warp_args, [], level=True, others=pyramids(1))
    refused(ValueError, "w: no pyramids", covis_args, [], level=True, pairs=[(0, 5)])
    refused(ValueError, "w: no pyramids", book_args, [], level=True, limit=0)
    # the call's other arguments before the level
    refused(ValueError, "w: 2 pyramids but 1 poses", map_args, pyramids(), level=True, poses=[EYE])
    refused(ValueError, "w: 2 raster pyramids but 1 sampled pyramids", warp_args, pyramids(), level=True, others=pyramids(1), transforms=[EYE])
    refused(ValueError, "w: a pose has an entry that is not finite", warp_args, pyramids(), level=9, transforms=[EYE, NAN])
    refused(ValueError, "w: a pair names a pyramid outside 0 .. 1", covis_args, pyramids(), level=1.0, pairs=[(0, 2)])
    refused(ValueError, "w: a pair names a pyramid outside 0 .. 1", covis_args, pyramids(), pairs=[(0, 2)], transforms=[NAN])
    refused(ValueError, "w: a pose has an entry that is not finite", covis_args, pyramids(), level=True, transforms=[NAN])
    refused(ValueError, "w: 3 pyramids, one call takes 2", book_args, pyramids(3), level=True, limit=2)
    # the level's type before its range, its range before the context -- pyramid by pyramid -- and both before what comes last
    for call in CALLERS:
        refused(TypeError, "w: level must be an integer", call, mixed, level=2.0)
        refused(ValueError, "w: a pyramid of 2 levels has no level 2", call, mixed, level=2)
        refused(ValueError, FOREIGN[call], call, pyramids(1, levels=3) + pyramids(1, OTHER, levels=3) + pyramids(1, levels=2), level=2)
        refused(ValueError, "w: a pyramid of 2 levels has no level 2", call, pyramids(1, levels=3) + pyramids(1, levels=2) + pyramids(1, OTHER, levels=3), level=2)
    refused(ValueError, "w: a pyramid of 2 levels has no level 2", map_args, pyramids(), level=2, lo=1.0, hi=0.0)
    refused(ValueError, "w: need min_depth <= max_depth (no NaN)", map_args, pyramids(), lo=float("nan"))
    # a warp's second pyramids: the level and the context of every one of them, then the sizes of the pairs
    small = [Pyramid(CTX, 2, Camera(16, 12)), Pyramid(CTX, 2)]
    refused(ValueError, "w: a pyramid of 1 levels has no level 1", warp_args, pyramids(), level=1, others=[small[0], Pyramid(CTX, 1)])
    refused(ValueError, "w: the pyramids belong to different contexts", warp_args, pyramids(), others=[small[0], Pyramid(OTHER)])
    refused(ValueError, "w: the pyramids of a pair differ in size", warp_args, pyramids(), others=small)
