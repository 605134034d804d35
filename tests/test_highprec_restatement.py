"""CPU: the oracle's voxel attributes, second bounce and directional mip chains (the three stages oracle/vct_oracle.h calls
"the build's own" definition) held to tests/highprec_ref.py, a float64 restatement written from the header's prose, by the
rule stated there (|byte - exact| <= 0.5 + eps, eps derived; at most 2 % left out near a discrete decision and those held
to 1 + eps), and to known answers written out by hand.  Scenes and volumes: tests/highprec_cases.py, shared with
tests/test_gpu_highprec.py, which holds the kernels to the same reference.  Every test prints its figures."""
import numpy as np
import pytest

import dynbouncecases as db
import dyncases as dc
import dynemiscases
import highprec_cases as hc
import highprec_ref as hp


def scene_layer(oracle, V, G, mesh=None):
    depth, vp = hc.shadow_for(G)
    return dc.layer(oracle, *(mesh or hc.static_mesh(G)), G=G, V=V, depth=depth, vp=vp)


# ---- bounce -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V, wrap, G, c", hc.BOUNCE_CASES)
def test_bounce(oracle, V, wrap, G, c):
    p = oracle.default_params(V, G=G, wrap_repeat=wrap, **hc.constants_kw(c))
    l0, alb, nrm = scene_layer(oracle, V, G)
    assert len(np.unique(l0.reshape(-1, 4), axis=0)) >= 20                # the raised map: level 0 is not one colour
    chain = oracle.build_mips(l0)
    out, steps = oracle.bounce(p, chain, alb, nrm, nthreads=4)
    assert (out != l0).any(-1).sum() >= 100
    r = hp.check_bounce(hp.params(p), chain, alb, nrm, out, steps, f"{V} wrap={wrap} G={G} constants={c}")
    print(r)
    assert r["steps"] == steps or r["left_out"] > 0


def test_bounce_over_a_merged_chain(oracle):
    """The input of the DYN kernels: mover A merged into the static layer, every voxel shaded with its owner's attributes."""
    V = 16
    S3, D3 = scene_layer(oracle, V, 150.0), scene_layer(oracle, V, 150.0, hc.mover())
    assert (D3[0][..., 3] > 0).sum() >= 50
    alb, nrm = db.owner(D3, S3)
    p = oracle.default_params(V, G=150.0)
    chain = oracle.build_mips(dc.merge(D3[0], S3[0]))
    out, steps = oracle.bounce(p, chain, alb, nrm)
    print(hp.check_bounce(hp.params(p), chain, alb, nrm, out, steps, "merged"))


def test_the_scenes_only_the_gpu_file_uses_stay_under_the_cap(oracle):
    """The dense 16^3 scene (k_bounce_bricks) and mover A at 16^3 and 64^3 without a shadow map, with and without its
    emission table: check_bounce asserts the left-out share; run here on the oracle's chains so that the cap is known to
    hold without a GPU."""
    p = oracle.default_params(16, G=150.0)
    l0, alb, nrm = dc.layer(oracle, *db.dense16_static(), V=16)
    chain = oracle.build_mips(l0)
    print("dense", hp.check_bounce(hp.params(p), chain, alb, nrm, *oracle.bounce(p, chain, alb, nrm, nthreads=4), "dense"))
    pos, mat, _ = mesh = dc.dynamic_mesh(dc.A)
    for V in (16, 64):
        p = oracle.default_params(V, G=150.0)
        S3, D3 = dc.layer(oracle, *dc.static_scene(), V=V), dc.layer(oracle, *mesh, V=V)
        alb, nrm = db.owner(D3, S3)
        for emission in (False, True):
            D = dynemiscases.add(D3[0], dynemiscases.dem(oracle, pos, mat, hc.EMISSION, V=V)) if emission else D3[0]
            chain = oracle.build_mips(dc.merge(D, S3[0]))
            what = f"mover A at {V}^3, emission={emission}"
            print(what, hp.check_bounce(hp.params(p), chain, alb, nrm, *oracle.bounce(p, chain, alb, nrm, nthreads=4), what))


# ---- directional mips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hc.VOLUMES)
@pytest.mark.parametrize("V", [8, 16, 32])
def test_directional_mips(oracle, V, kind):
    l0 = hc.volume(kind, V)
    aniso = oracle.build_mips_aniso(l0)
    x = hp.aniso_chain_from_bytes(l0, aniso)                       # every level from the previous level's bytes
    worst = hp.agree(aniso, x, hp.EPS_MIP, f"{kind} {V}")
    ties = int((np.abs(x - np.floor(x) - 0.5) < 1e-9).sum())
    print(kind, V, "largest |b - x| - 0.5:", worst, "exact ties:", ties, "of", x.size, "eps", hp.EPS_MIP)
    assert len(np.unique(aniso.reshape(6, -1), axis=0)) == 6        # the six chains differ


# ---- directional trace --------------------------------------------------------------------------------------------------
TRACE_CASES = [(f, wrap, c) for f in ("random", "coherent") for wrap in (1, 0) for c in (0, 1, 2)]


@pytest.fixture(scope="module")
def traced_volume(oracle):
    l0 = hc.volume("noise", 16)
    return oracle.build_mips(l0), oracle.build_mips_aniso(l0)


@pytest.mark.parametrize("frame, wrap, c", TRACE_CASES)
def test_directional_trace(oracle, traced_volume, frame, wrap, c):
    """The oracle's raw fp32 cones against the float64 cones: the figure CONE_DEV_MEASURED comes from here, and the GPU
    file's bound is four times it."""
    chain, aniso = traced_volume
    planes = hc.frames()[frame]
    p = oracle.default_params(16, wrap_repeat=wrap, camera_pos=hc.CAMERA, **hc.constants_kw(c, hc.TRACE_CONSTANTS))
    r = oracle.trace_aniso(p, chain, aniso, planes, want_cones=True)
    iso = oracle.trace(p, chain, planes, want_cones=True)
    assert (r["cones"] != iso["cones"]).any(-1).sum() >= 500       # the directional route shows
    got = hp.check_cones(hp.params(p), chain, aniso, planes, hc.CAMERA, r["cones"], r["steps"],
                         bound=hp.CONE_DEV_MEASURED, what=f"{frame} wrap={wrap} constants={c}")
    print(frame, wrap, c, got)
    assert got["marched"] >= 2000 and r["total_steps"] == got["steps"]


# ---- known answers: directional mips ------------------------------------------------------------------------------------
def test_known_directional_blocks(oracle):
    """Each block of highprec_cases.known_blocks() tiled over 4^3: all eight parents of a chain are the hand-written texel."""
    for blk, want in hc.known_blocks():
        l0 = hc.tiled(blk, 4)
        aniso = oracle.build_mips_aniso(l0)
        hp.agree(aniso, hp.aniso_chain_from_bytes(l0, aniso), hp.EPS_MIP, "known block")     # the reference: the same
        for d, texel in want.items():
            assert (aniso[d, :8] == texel).all(), (blk.tolist(), d, aniso[d, 0], texel)


# ---- known answers: directional sampling --------------------------------------------------------------------------------
def constant_chains(V, values):
    """Six directional chains, chain d everywhere values[d] in all four channels."""
    n = hp_chain_texels(V) - V ** 3
    return np.repeat(np.asarray(values, np.uint8)[:, None, None], n, 1).repeat(4, 2)


def hp_chain_texels(V):
    return sum((V >> k) ** 3 for k in range(int(np.log2(V)) + 1))


def one_pixel(normal):
    """A pixel at the origin whose frame has N = normal: cone 0 marches along it."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    h = np.array([0.0, 1.0, 0.0]) if abs(n[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    t = np.cross(h, n) / np.linalg.norm(np.cross(h, n))
    g = np.zeros((23, 1), np.float32)
    g[3:6, 0], g[6:9, 0], g[9:12, 0], g[12:15, 0] = n * 0.05, t * 0.05, np.cross(n, t) * 0.05, n
    g[15:19, 0] = (0.5, 0.5, 0.5, 1.0)
    return g


@pytest.mark.parametrize("side", ["oracle", "reference"])
def test_known_directional_sampling(oracle, side):
    V = 16
    p = oracle.default_params(V, camera_pos=hc.CAMERA)
    chain = np.zeros((hp_chain_texels(V), 4), np.uint8)          # an empty isotropic chain: only levels >= 1 give anything

    def cone0(normal, values):
        an = constant_chains(V, values)
        if side == "oracle":
            return oracle.trace_aniso(p, chain, an, one_pixel(normal), want_cones=True)["cones"][0, 0].astype(np.float64)
        return hp.frame_cones(hp.params(p), chain, an, one_pixel(normal), hc.CAMERA)[0][0, 0]
    base = [10, 20, 30, 40, 50, 60]                              # chain d = 2 * axis + sign holds base[d] everywhere
    for axis in range(3):
        for sign in (0, 1):
            d = 2 * axis + sign
            n = np.zeros(3)
            n[axis] = 1.0 - 2.0 * sign
            got = cone0(n, base)
            assert got[3] > 0
            others = [v if i == d else 255 - v for i, v in enumerate(base)]
            assert np.array_equal(got, cone0(n, others)), (d, "another chain contributes")
            alone = [v if i == d else 0 for i, v in enumerate(base)]
            assert np.array_equal(got, cone0(n, alone))
            changed = list(base)
            changed[d] += 5
            assert (cone0(n, changed) > got).all(), (d, "the matching chain does not contribute")
    # a diagonal: the mean of its three chains -- (12 + 30 + 63) / 3 = 35 for (+, +, -); dir^2 = 1/3 each
    diag = [12, 20, 30, 40, 50, 63]
    got = cone0((1.0, 1.0, -1.0), diag)
    assert got[3] > 0 and np.allclose(got, cone0((1.0, 1.0, -1.0), [35] * 6), rtol=1e-5, atol=0)
    assert not np.allclose(got, cone0((1.0, 1.0, -1.0), [34] * 6), rtol=1e-3, atol=0)
    assert not np.allclose(got, cone0((1.0, 1.0, 1.0), diag), rtol=1e-3, atol=0)          # the sign picks the chain


# ---- known answers: bounce ----------------------------------------------------------------------------------------------
def hand_volume(V=16):
    """A few opaque voxels far apart, with axis normals; everything else empty."""
    l0, alb, nrm = (np.zeros((V, V, V, 4), np.uint8) for _ in range(3))
    vox = {(8, 8, 8): (128, 255, 128), (3, 12, 5): (128, 1, 128), (12, 3, 10): (255, 128, 128), (5, 5, 13): (128, 128, 1)}
    for (z, y, x), n in vox.items():
        l0[z, y, x] = (60, 120, 180, 255)
        alb[z, y, x] = (230, 77, 64, 255)
        nrm[z, y, x] = n + (255,)
    return l0, alb, nrm, list(vox)


def test_known_bounce_unchanged_outputs(oracle):
    V = 16
    p = oracle.default_params(V, G=150.0)
    l0, alb, nrm, vox = hand_volume(V)
    # 16^3, G = 150: vs = 9.375; a cone nothing stops runs dist = 9.375 -> 20.19 -> 43.49 -> 93.67: three steps, six cones
    out, steps = oracle.bounce(p, oracle.build_mips(l0), alb, nrm)
    assert steps == 18 * len(vox)
    assert np.array_equal(out[..., 3], l0[..., 3])
    # level 0 with rgb all zero, whatever the occlusion: every byte as it was
    dark = l0.copy()
    dark[..., :3] = 0
    dark[2:14:3, 2:14:3, 2:14:3, 3] = 200                        # occluders without colour
    for v in vox:
        dark[v][3] = 255
    out, _ = oracle.bounce(p, oracle.build_mips(dark), alb, nrm)
    assert np.array_equal(out, dark)
    # a lit volume (so that the bounce adds something) ...
    lit = l0.copy()
    lit[::2, ::2, ::2] = np.where(lit[::2, ::2, ::2][..., 3:] == 0, np.uint8([[200, 220, 240, 255]]), lit[::2, ::2, ::2])
    chain = oracle.build_mips(lit)
    out, steps = oracle.bounce(p, chain, alb, nrm)
    assert all((out[v][:3] > lit[v][:3]).all() for v in vox)
    assert np.array_equal(out[..., 3], lit[..., 3])                                  # alpha always the input's
    untouched = np.ones((V, V, V), bool)
    for v in vox:
        untouched[v] = False
    assert np.array_equal(out[untouched], lit[untouched])                            # no stored normal: copied
    # ... albedo attribute zero leaves the voxel unchanged, the others as before
    alb0 = alb.copy()
    alb0[vox[1]][:3] = 0
    out0, steps0 = oracle.bounce(p, chain, alb0, nrm)
    assert np.array_equal(out0[vox[1]], lit[vox[1]]) and steps0 == steps
    assert all(np.array_equal(out0[v], out[v]) for v in vox if v != vox[1])
    # ... a stored normal of (128, 128, 128) is copied and marches nothing
    nrm0 = nrm.copy()
    nrm0[vox[2]][:3] = 128
    outn, stepsn = oracle.bounce(p, chain, alb, nrm0)
    mine = hp.bounce(hp.params(p), chain, alb, nrm)
    its_cones = int(mine["steps"][[tuple(i) == vox[2] for i in mine["idx"].tolist()]][0])
    assert np.array_equal(outn[vox[2]], lit[vox[2]]) and 6 <= its_cones <= 18 and stepsn == steps - its_cones
    hp.check_bounce(hp.params(p), chain, alb, nrm, out, steps, "hand volume, lit")


def test_known_bounce_frame(oracle):
    # the frame by hand: helper (1,0,0) for n = +-y, (0,1,0) for n = +x; t = normalize(helper x n), b = n x t
    n = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])
    t, b = hp.bounce_frame(n, np.abs(n[:, 1]) < 0.9)
    assert np.array_equal(t, [[0, 0, 1], [0, 0, -1], [0, 0, -1]]) and np.array_equal(b, [[1, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert np.allclose((t * n).sum(1), 0) and np.allclose(np.cross(n, t), b) and np.allclose(np.linalg.det(np.stack([t, b, n], 2)), 1)
    V = 16
    p = oracle.default_params(V, G=150.0, wrap_repeat=0)
    pr = hp.params(p)

    def gain(normal_bytes, lit_voxels, at=(8, 8, 8)):
        l0, alb, nrm = (np.zeros((V, V, V, 4), np.uint8) for _ in range(3))
        l0[at], alb[at], nrm[at] = (0, 0, 0, 255), (255, 255, 255, 255), tuple(normal_bytes) + (255,)
        for z, y, x in lit_voxels:
            l0[z, y, x] = (255, 255, 255, 255)
        chain = oracle.build_mips(l0)
        out, steps = oracle.bounce(p, chain, alb, nrm)
        hp.check_bounce(pr, chain, alb, nrm, out, steps, "frame")
        return int(out[at][0])
    # lit from one side only (clamp-to-edge): the upper-x half of the volume is lit, the voxel sits at x = 3.  Facing away
    # its samples stay at x <= 2.5 voxels: level 2 reads texels 0 and 1 (x < 8), levels 3 and 4 are never reached past
    # texel 0 (lod <= 2.42, clamp-to-edge) -- nothing lit; facing it gains
    half = [(z, y, x) for z in range(V) for y in range(V) for x in range(8, V)]
    assert gain((255, 128, 128), half, (8, 8, 3)) > 20 and gain((1, 128, 128), half, (8, 8, 3)) == 0
    # n = +y, so b = +x and t = +z: cone 1 = (0, .866, .5) leaves towards +x, cones 3 and 4 towards -x and 36 degrees to
    # either side of it.  The first sample (dist = vs, from P + n * vs) of cone 1 lies at (+.866, +1.5, 0) voxels: weight
    # .15 * .866 on the texel one to the +x side; of cones 3, 4 at (-.70, +1.5, +-.51): 2 * .15 * .70 * .49 on the -x one;
    # cones 2, 5 at (+.27, +1.5, +-.82) add 2 * .15 * .27 * .18 to the +x side.  .144 against .103: +x gains more.
    plus = gain((128, 255, 128), [(8, 9, 9), (8, 10, 9)])
    minus = gain((128, 255, 128), [(8, 9, 7), (8, 10, 7)])
    print("lit on the +b side", plus, "on the -b side", minus)
    assert plus > minus > 0
    # and the other helper's case: n = +x, b = +y
    assert gain((255, 128, 128), [(8, 9, 9), (8, 9, 10)]) > gain((255, 128, 128), [(8, 7, 9), (8, 7, 10)]) > 0


# ---- known answers: attributes ------------------------------------------------------------------------------------------
# As float32 0.9 is 0.899999976: times 255 exactly 229.4999939, which fp32 rounds to 229.5 -- the byte is 230, 6.1e-6 LSB
# beyond the half and inside EPS_UNORM.  0.3 is 0.300000012: 76.500003 -> 77.  From decimal literals both would be ties.
ALBEDO = (0.9, 0.3, 0.25, 1.0)
ALBEDO_BYTES = (230, 77, 64)


@pytest.mark.parametrize("name", list(hc.KNOWN_TRIANGLES))
def test_known_attribute_normals(oracle, name):
    tri, want = hc.KNOWN_TRIANGLES[name]
    V = 16
    l0, alb, nrm = dc.layer(oracle, *hc.tri_mesh([tri], [ALBEDO]), V=V)
    occ = l0[..., 3] > 0
    assert occ.sum() >= 4 and np.array_equal(occ, nrm[..., 3] == 255) and np.array_equal(occ, alb[..., 3] == 255)
    assert not nrm[~occ].any() and not alb[~occ].any()
    assert (nrm[occ][:, :3] == want).all(), (name, np.unique(nrm[occ], axis=0), want)
    assert (alb[occ][:, :3] == ALBEDO_BYTES).all(), np.unique(alb[occ], axis=0)
    assert tuple(hp.quantise_normal(hp.face_normal(tri))) == want
    worst = hp.agree(np.array(ALBEDO_BYTES), hp.albedo_lsb(ALBEDO[:3]), hp.EPS_UNORM, "albedo")
    assert 0 < worst < 1e-5                                       # the double rounding of 0.9f * 255, and nothing more


def test_attribute_ranges_on_a_scene(oracle):
    l0, alb, nrm = dc.layer(oracle, *dc.static_scene(), V=32)
    occ = l0[..., 3] > 0
    assert occ.sum() >= 1000
    assert (nrm[occ] >= 1).all() and (nrm[occ][:, 3] == 255).all() and (alb[occ][:, 3] == 255).all()
    assert not nrm[~occ].any() and not alb[~occ].any() and not l0[~occ].any()


def test_two_coplanar_triangles_with_two_materials(oracle):
    q = [[-500.0, -400.0, 100.0], [450.0, -400.0, 100.0], [450.0, 500.0, 100.0], [-500.0, 500.0, 100.0]]
    mesh = hc.tri_mesh([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], [ALBEDO, (0.2, 0.8, 0.6, 1.0)], [0, 1])
    one = [dc.layer(oracle, *hc.tri_mesh([t], [a]), V=16)[0][..., 3] > 0
           for t, a in (([q[0], q[1], q[2]], ALBEDO), ([q[0], q[2], q[3]], ALBEDO))]
    l0, alb, nrm = dc.layer(oracle, *mesh, V=16)
    occ = l0[..., 3] > 0
    shared = one[0] & one[1]
    assert shared.sum() >= 4 and np.array_equal(occ, one[0] | one[1])
    assert (nrm[occ][:, :3] == (128, 128, 255)).all()
    m0, m1 = np.array(ALBEDO_BYTES), np.array((51, 204, 153))
    assert (alb[one[0] & ~shared][:, :3] == m0).all() and (alb[one[1] & ~shared][:, :3] == m1).all()
    s = alb[shared][:, :3].astype(np.int64)
    assert (s >= np.minimum(m0, m1)).all() and (s <= np.maximum(m0, m1)).all()
    assert ((s != m0).any(-1) & (s != m1).any(-1)).sum() >= 1     # a mean somewhere, not one material's colour
