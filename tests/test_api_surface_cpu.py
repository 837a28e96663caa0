"""The names the post-training modules expose: evaluate, inference, topology and holes still carry every public name they carried before
evaluate.py was split by subject, and what evaluate re-exports is the object of its home module, not a copy.  The lists are those of
the commit before the split, as `vars(module)` gave them (no leading underscore, not a module), without what was visible only because
a module imported it for its own use: the names of `typing` and `__future__`, and the check helpers of the private `_args` module."""
import importlib

import pytest

NAMES = {
    "evaluate": [
        "ALIGN_MODES", "CLOUD_STATS", "CloudMetrics", "CloudNN", "DepthMetrics", "MAX_DEPTH", "MAX_SURFACE_PAIRS", "MAX_THRESHOLDS",
        "METRICS", "MIN_DEPTH", "Mesh", "Meshing", "REGISTER_HISTORY", "REGISTER_METRICS", "REGISTER_MODES", "REGISTER_NOT_PD",
        "REGISTER_OK", "REGISTER_REVERTED", "REGISTER_TOO_FEW", "Registration", "RegistrationResult", "SURFACE_STATS",
        "SequenceEvaluation", "SurfaceMetrics", "SurfaceNN", "align_trajectory", "ate", "clean_mesh", "cloud_metrics", "depth_metrics",
        "evaluate_sequence", "mesh_topology", "metrics_from_stats", "nearest_neighbors", "point_to_surface", "reconstruction_metrics",
        "register_accumulate", "register_clouds", "rpe", "summarize", "surface_metrics", "surface_reconstruction_metrics",
        "transform_cloud"],
    "inference": [
        "CleanedMesh", "CloudNormals", "Consistency", "ConsistencyResult", "FusedCloud", "HoleFill", "MAX_DEPTH", "Mesh", "MeshTopology",
        "MeshViews", "Meshing", "REFINE_BAD_EDGE", "REFINE_NOT_PD", "REFINE_OK", "REFINE_REVERTED", "REFINE_TOO_FEW", "Reconstruction",
        "Refinement", "RefinementResult", "Render", "RenderedViews", "SurfelViews", "TsdfVolume", "backproject", "check_consistency",
        "check_refinement", "check_render", "clean_mesh", "cloud_normals", "extract_mesh", "fill_holes", "filter_depths",
        "fuse_point_cloud", "fuse_tsdf", "fusion_grid", "integrate_trajectory", "mesh_topology", "pose_to_matrix4",
        "reconstruct_sequence", "refine_accumulate", "refine_edges", "refine_trajectory", "render_cloud", "render_fused", "render_mesh",
        "render_surfels", "rigid_inverse", "run_networks", "stitch_point_cloud", "tsdf_voxels", "write_ply"],
    "topology": ["CleanedMesh", "MAX_FACES", "Mesh", "MeshTopology", "clean_mesh", "mesh_topology"],
    "holes": ["FILLED", "HoleFill", "MAX_VERTICES", "Mesh", "MeshTopology", "NOT_SIMPLE", "TOO_LONG", "UNMEASURED", "fill_holes"],
}
HOMES = ("trajectory", "cloud_eval", "registration", "surface_eval", "fusion", "topology")      # where evaluate's re-exports live


@pytest.mark.parametrize("module", sorted(NAMES))
def test_every_public_name_is_still_there(module):
    mod = importlib.import_module(f"coivo_amd.{module}")
    missing = [n for n in NAMES[module] if not hasattr(mod, n)]
    assert not missing, f"coivo_amd.{module} lost {missing}"


def test_evaluate_re_exports_the_home_modules_own_objects():
    E = importlib.import_module("coivo_amd.evaluate")
    homes = [importlib.import_module(f"coivo_amd.{m}") for m in HOMES]
    own = {"DepthMetrics", "METRICS", "MIN_DEPTH", "MAX_DEPTH", "SequenceEvaluation", "depth_metrics", "evaluate_sequence", "summarize"}
    seen = set()
    for name in NAMES["evaluate"]:
        for home in homes:
            if name in vars(home):
                assert getattr(E, name) is getattr(home, name), f"evaluate.{name} is not {home.__name__}.{name}"
                seen.add(name)
    assert seen | own == set(NAMES["evaluate"]), sorted(set(NAMES["evaluate"]) - seen - own)
    for name in ("align_trajectory", "cloud_metrics", "register_clouds", "point_to_surface"):      # defined there, not passed through
        assert getattr(E, name).__module__ in {h.__name__ for h in homes[:4]}
    assert E.depth_metrics.__module__ == E.__name__ and E.evaluate_sequence.__module__ == E.__name__
