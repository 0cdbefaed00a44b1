"""GPU tier (-m gpu): the role planes ensure_roles builds for a frame list that mixes every source a frame's planes can be derived
from, in ONE call -- reached through dvo_hip_frames_prepare (the build stream, the flavours a small batch gets: taps A + B and, where
the level has one, plane C) and through a match (the main stream, option "resident" 0: plane C wherever a window or small sweep reads
it).  Every frame ends with the planes of a twin: a frame of the same pixels ingested alone straight into the role.

What the comparison sees.  dvo_hip_frame_download_plane reads the taps A + B (the six planes of a level), dvo_hip_frame_select without a
mask the selection count the reference role left; the C-ABI has no download of plane C or of plane R.  So the taps are compared bit
for bit plane by plane, and planes C and R -- of either route -- through what reads them: a match whose records must be those of the
twins' match, bit for bit (on the prepare route a match that finds nothing left to build on the prepared frames), and plane R through
its count as well.

The list, and the branch of ensure_roles each entry is there for (general per-level path; level 0 unless said otherwise):
  c_only       current-role ingest in a batch of 32 frames: plane C alone where level 0 has one (96 x 64), else the taps.
               current: A + B from C (prepare); reference: R from C.  "Only been a current frame", flavour C.
  ab_only      current-role ingest under option "variant" 5 (no window sweep: the taps alone), used under the default schedule.
               current: C from A (where level 0 has a C); reference: selection over A + B.  "Only been a current frame", flavour A + B.
  raw_only     created from raw planes, no role: everything from the frame's raw copy (k_build_from_raw over one level).
  float        created from float planes: level 0 from the planes I / Z like levels >= 1 of every other frame.
  other_scale  a raw-copy frame of another depth scale: one launch takes one scale, so it is left to the second pass.
  raw_only again: the second visit of a frame listed twice needs nothing any more.
Levels >= 1 of every frame come from the float planes, sorted by what each frame lacks (the 32-frame ingest has prepared c_only's).
At 131 x 97 no level has a plane C and no ingest runs in strips: k_derive_levels serves a single level."""
import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import datagen

pytestmark = pytest.mark.gpu

SHAPES = [(96, 64, 3), (131, 97, 2)]
KINDS = ("c_only", "ab_only", "raw_only", "float", "other_scale")
ORDER = (0, 1, 2, 3, 4, 2)                   # raw_only is listed twice
SCALE = {"other_scale": 1.0 / 1000.0}         # every other frame: 1 / 5000
PLANES = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
ITHR, DTHR = 8.0, 0.02
DEFAULT_VARIANT = 8


def scale_of(kind):
    return SCALE.get(kind, 1.0 / 5000.0)


def float_planes(grey, depth):
    z = depth.astype(np.float32) * np.float32(1.0 / 5000.0)
    z[depth == 0] = np.nan
    return np.ascontiguousarray(grey.astype(np.float32)), z


class Scene:
    """One context, one camera and the pixels of the five frames, as a reference set (`ref`) and a current set (`cur`)."""

    def __init__(self, w, h, levels):
        self.w, self.h, self.levels = w, h, levels
        self.cfg = d.Config(FirstLevel=levels - 1, LastLevel=0, IntensityDerivativeThreshold=ITHR, DepthDerivativeThreshold=DTHR)
        self.ctx = d.Context(0)
        self.ctx.set_option("resident", 0)   # (the launch path whatever the frames hold: the schedule must not depend on how a frame was built)
        b = datagen.synth_batch(811, len(KINDS), w, h)
        self.cam = d.RgbdCameraPyramid(w, h, b["K"], self.ctx)
        self.cam.build(levels)
        self.pixels = {side: [(np.ascontiguousarray(b["grey_" + side][k]), np.ascontiguousarray(b["depth_" + side][k])) for k in range(len(KINDS))]
                       for side in ("ref", "cur")}
        self.dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)

    def blank(self):
        return self.cam.create_raw(*self.dummy)

    def mixed(self, side):
        """The five frames in the states the module's docstring lists, and what has to outlive them."""
        px = self.pixels[side]
        crowd = [self.blank() for _ in range(32)]
        d.update_raw_host_batch(crowd, [px[0][0]] + [self.dummy[0]] * 31, [px[0][1]] + [self.dummy[1]] * 31, role="current", config=self.cfg)
        ab = self.blank()
        self.ctx.set_option("variant", 5)
        d.update_raw_host_batch([ab], [px[1][0]], [px[1][1]], role="current", config=self.cfg)
        d.upload_wait(self.ctx)
        self.ctx.set_option("variant", DEFAULT_VARIANT)
        raw = self.cam.create_raw(*px[2])
        flt = self.cam.create(*float_planes(*px[3]))
        other = self.cam.create_raw(*px[4], depth_scale=scale_of("other_scale"))
        return [crowd[0], ab, raw, flt, other], crowd

    def twins(self, side, role):
        """A frame per kind of the same pixels, ingested alone straight into `role`."""
        out = []
        for k, kind in enumerate(KINDS):
            f = self.blank()
            g, z = self.pixels[side][k]
            if kind == "float":
                i32, z32 = float_planes(g, z)
                d.update_f32_host_batch([f], [i32], [z32], role=role, config=self.cfg)
            else:
                d.update_raw_host_batch([f], [g], [z], depth_scale=scale_of(kind), role=role, config=self.cfg)
            d.upload_wait(self.ctx)
            out.append(f)
        return out

    def listed(self, frames):
        return [frames[k] for k in ORDER]


def records(out):
    """What a match returned, as bytes."""
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations", "entropy"))


def counts_of(scene, f):
    return [d.PointSelection(f, ITHR, DTHR).select(l) for l in range(scene.levels)]


def assert_same_frames(scene, got, want, what):
    """The six downloadable planes (the taps A + B) of every level bit for bit, and the selection counts."""
    for k, kind in enumerate(KINDS):
        for l in range(scene.levels):
            for name in PLANES:
                a, b = np.array(getattr(got[k].level(l), name)), np.array(getattr(want[k].level(l), name))
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, kind, l, name)
        got_counts, want_counts = counts_of(scene, got[k]), counts_of(scene, want[k])
        print(what, kind, "selection counts", got_counts, want_counts)
        assert got_counts == want_counts, (what, kind)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s[:2])
def scene(request):
    s = Scene(*request.param)
    yield s
    s.ctx.close()


@pytest.mark.parametrize("role", ["current", "reference"])
def test_prepare_of_a_mixed_list_equals_frames_ingested_alone(scene, role):
    """dvo_hip_frames_prepare over the mixed list (ensure_roles, eager): the planes and counts of the twins."""
    frames, keep = scene.mixed("ref")
    twins = scene.twins("ref", role)
    d.prepare_roles_batch(scene.listed(frames), role, scene.cfg)
    # planes C and R as the build stream left them, through what reads them: a match against partners in the other role finds nothing
    # to build on the prepared frames (a list this small is prepared with every flavour) and returns the records of the twins' match
    other = "reference" if role == "current" else "current"
    partners = scene.listed(scene.twins("cur", other))
    trk = d.DenseTracker(scene.cfg, scene.ctx)
    pair_up = (lambda mine: (partners, mine)) if role == "current" else (lambda mine: (mine, partners))
    scene.ctx.set_option("variant", DEFAULT_VARIANT)          # (naming the schedule clears its history: both matches start alike)
    want = trk.match_batch_arrays(*pair_up(scene.listed(twins)))
    scene.ctx.set_option("variant", DEFAULT_VARIANT)
    got = trk.match_batch_arrays(*pair_up(scene.listed(frames)))
    assert records(got) == records(want)
    if role == "reference":
        # (the counts first: they are what the call above left; a download derives the current role and leaves the reference role alone)
        for k, kind in enumerate(KINDS):
            assert counts_of(scene, frames[k]) == counts_of(scene, twins[k]), kind
    assert_same_frames(scene, frames, twins, "prepare " + role)
    del keep


def test_match_of_mixed_lists_equals_frames_ingested_alone(scene):
    """dvo_hip_match_batch over a mixed reference list and a mixed current list (ensure_roles on the main stream, both roles): the
    records of the twins' match, bit for bit, then the planes and counts."""
    refs, keep_r = scene.mixed("ref")
    curs, keep_c = scene.mixed("cur")
    twin_refs, twin_curs = scene.twins("ref", "reference"), scene.twins("cur", "current")
    trk = d.DenseTracker(scene.cfg, scene.ctx)
    scene.ctx.set_option("variant", DEFAULT_VARIANT)          # (naming the schedule clears its history: both matches start alike)
    want = trk.match_batch_arrays(scene.listed(twin_refs), scene.listed(twin_curs))
    scene.ctx.set_option("variant", DEFAULT_VARIANT)
    got = trk.match_batch_arrays(scene.listed(refs), scene.listed(curs))
    print("iterations", got["n_iterations"], want["n_iterations"])
    assert records(got) == records(want)
    assert records(got) != records(trk.match_batch_arrays(scene.listed(twin_curs), scene.listed(twin_refs)))   # (the pairs are no identities)
    for k, kind in enumerate(KINDS):
        assert counts_of(scene, refs[k]) == counts_of(scene, twin_refs[k]), kind
    assert_same_frames(scene, refs, twin_refs, "match, reference list")
    assert_same_frames(scene, curs, twin_curs, "match, current list")
    del keep_r, keep_c
