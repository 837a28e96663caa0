"""coivo_amd.inference stays the one place to import the post-training entry points from, whichever module holds them: every name
it exported before the split into fusion / consistency / refine / render / ply is still there and is the same object as in its home
module, and localize and evaluate can each be the first module imported."""
import importlib
import os
import subprocess
import sys

import pytest

# the names coivo_amd.inference defined before the split (every top-level definition without a leading underscore), by home module
SURFACE = {
    "coivo_amd._args": ["MAX_DEPTH"],
    "coivo_amd.inference": ["pose_to_matrix4", "integrate_trajectory", "backproject", "stitch_point_cloud", "Reconstruction",
                            "run_networks", "reconstruct_sequence"],
    "coivo_amd.fusion": ["FusedCloud", "fusion_grid", "fuse_point_cloud", "TsdfVolume", "Mesh", "Meshing", "fuse_tsdf", "extract_mesh",
                         "CloudNormals", "cloud_normals"],
    "coivo_amd.consistency": ["Consistency", "ConsistencyResult", "filter_depths"],
    "coivo_amd.refine": ["Refinement", "RefinementResult", "REFINE_OK", "REFINE_TOO_FEW", "REFINE_NOT_PD", "REFINE_REVERTED",
                         "REFINE_BAD_EDGE", "refine_accumulate", "refine_edges", "refine_trajectory"],
    "coivo_amd.render": ["Render", "RenderedViews", "render_cloud", "SurfelViews", "render_surfels", "render_fused", "MeshViews",
                         "render_mesh"],
    "coivo_amd.ply": ["write_ply"],
}
NAMES = [(home, name) for home, names in SURFACE.items() for name in names]


def test_the_list_is_the_forty_names():
    assert len(NAMES) == 40 and len({n for _, n in NAMES}) == 40


@pytest.mark.parametrize("home,name", NAMES)
def test_name_is_importable_from_inference_and_is_its_home_modules_object(home, name):
    from coivo_amd import inference
    assert hasattr(inference, name), name
    assert getattr(inference, name) is getattr(importlib.import_module(home), name)


def test_refine_constants_keep_their_values():
    from coivo_amd import inference as I
    assert (I.REFINE_OK, I.REFINE_TOO_FEW, I.REFINE_NOT_PD, I.REFINE_REVERTED, I.REFINE_BAD_EDGE) == (0, 1, 2, 3, 4)
    assert I.MAX_DEPTH == 10.0


def test_isinstance_holds_across_modules():
    import torch
    from coivo_amd import fusion, inference
    cloud = inference.FusedCloud(torch.zeros(1, 3), None, torch.ones(1, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int32),
                                 (0.0, 0.0, 0.0), (8, 8, 8), 0.02, 1, 0, 1, 1)
    assert isinstance(cloud, fusion.FusedCloud)


@pytest.mark.parametrize("first", ["localize", "evaluate", "inference", "render", "fusion"])
def test_module_can_be_imported_first(first):
    """A fresh interpreter: no import order has papered over a cycle (localize takes align_trajectory from trajectory, not evaluate)."""
    code = (f"import coivo_amd.{first} as m, sys; import coivo_amd.inference as I, coivo_amd.localize as L, coivo_amd.evaluate as E; "
            "assert I.localize is L and L.align_trajectory is E.align_trajectory and E.inference is I; print('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
