"""The inputs and expected values of the dynamic mesh's emission (include/vct.h "dynamic mesh", Emission), NumPy only.
Test infrastructure: the scenes are tests/dyncases.py's, the rule is tests/emission_ref.py's applied to the dynamic mesh
alone -- DEm = oracle.voxelize_conservative(dynamic mesh, pad4(table), no shadow map), D' = min(255, D + DEm) per byte
with D's alpha -- and the chain is dyncases.merge(D', S)."""
import numpy as np

import dyncases as dc
import emission_ref

# per material of dyncases' three: one glows below 1, one not at all, one has a channel above 1 (it saturates alone)
EM = np.array([[0.9, 0.35, 0.1], [0.0, 0.0, 0.0], [0.25, 2.0, 0.6]], np.float32)
ONE = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 2.0, 0.6]], np.float32)       # a second table: material 2 alone


def dem(oracle, pos, mat, table=EM, ms=dc.MS, G=dc.G, V=dc.V):
    """DEm, uint8 [V, V, V, 4]: the mesh voxelized alone with the table as its colours and no shadow map."""
    p = oracle.default_params(V, G=G)
    return oracle.voxelize_conservative(p, oracle.make_scene(pos, mat, emission_ref.pad4(table), ms))


def add(D, DEm):
    """D' = D + DEm per byte with saturation, alpha D's."""
    out = D.copy()
    out[..., :3] = np.minimum(255, D[..., :3].astype(np.int32) + DEm[..., :3].astype(np.int32)).astype(np.uint8)
    return out


def non_degeneracy(D, DEm, table=EM):
    """emission_ref.non_degeneracy's counts, and the dynamic voxels whose DEm is all zero (D' = D there)."""
    n = emission_ref.non_degeneracy(D, DEm, table)
    n["dynamic_voxels"] = int((D[..., 3] > 0).sum())
    n["zero_emission"] = int(((D[..., 3] > 0) & (DEm[..., :3] == 0).all(-1)).sum())
    return n


def assert_non_degenerate(D, DEm, table=EM):
    """The lower bounds under which a comparison with D' cannot pass vacuously."""
    n = non_degeneracy(D, DEm, table)
    assert n["same_alpha"], n
    assert n["saturating"] >= 100 and n["both"] >= 100 and n["mixed_values"] >= 5 and n["zero_emission"] >= 50, n
    return n
