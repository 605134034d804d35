"""The second bounce over the dynamic mesh (include/vct.h "dynamic mesh", vct_set_dynamic_bounce): the expected chains from
the CPU oracle, NumPy only.  With the layer's volumes (D, Da, Dn) and the static resolve's (S, Sa, Sn)

    level0' = vcto_bounce(chain0 = mips(merged level 0), where(D.a > 0, Da, Sa), where(D.a > 0, Dn, Sn))

-- a voxel the layer occupies is shaded with the layer's albedo and normal, every other one with the static ones, and
both gather from the merged chain.  Scenes: tests/dyncases.py; the dense 16^3 scene is the seed-77 scene of
tests/test_gpu_parity.py test_second_bounce_dense_scene_overflows_the_voxel_list."""
import numpy as np

import dyncases as dc


def owner(D3, S3):
    """(albedo, normal) of every voxel's owner."""
    d = (D3[0][..., 3] > 0)[..., None]
    return np.where(d, D3[1], S3[1]), np.where(d, D3[2], S3[2])


def bounce(oracle, p, l0, alb, nrm):
    """(level 0 after the bounce, steps) over the chain of l0."""
    return oracle.bounce(p, oracle.build_mips(l0), alb, nrm, nthreads=8)


def expected(oracle, D3, S3, l0=None, p=None):
    """The bounce with the switch on: (level 0', steps).  l0: the lit merged level 0 where lights or emission changed it."""
    p = p or oracle.default_params(D3[0].shape[0], G=dc.G)
    return bounce(oracle, p, dc.merge(D3[0], S3[0]) if l0 is None else l0, *owner(D3, S3))


def static_attributes(oracle, D3, S3, p=None):
    """What a bounce that knew the static pools only would give over the merged chain."""
    p = p or oracle.default_params(D3[0].shape[0], G=dc.G)
    return bounce(oracle, p, dc.merge(D3[0], S3[0]), S3[1], S3[2])


def detached(oracle, S3, p=None):
    p = p or oracle.default_params(S3[0].shape[0], G=dc.G)
    return bounce(oracle, p, S3[0], S3[1], S3[2])


def differing(a, b):
    return (a != b).any(-1)


def dense16_static():
    """The dense 16^3 scene: more than V^3 / 8 voxels occupied, the voxel list overflows."""
    r = np.random.default_rng(77)
    ntri = 1500
    c = r.uniform(-1400, 1400, (ntri, 1, 3))
    pos = (c + r.normal(scale=260.0, size=(ntri, 3, 3))).astype(np.float32)        # big triangles: a dense grid
    mat = r.integers(0, 3, ntri).astype(np.int32)
    alb = r.uniform(0.2, 0.9, (3, 4)).astype(np.float32)
    return pos.reshape(-1, 9), mat, alb


def zero_normal(nrm):
    return (nrm[..., :3] == 128).all(-1)
