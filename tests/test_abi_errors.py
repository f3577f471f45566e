"""The argument checks of every f-row entry point, of the a-row stage entries
that take only pointers and scalars, and of the encoder row's weight, encoder,
attention, timing, layout and plan entries, replayed against a recorded
table (tests/golden/abi_errors/abi_errors.json) -- no GPU needed: every call
here is rejected on the host before the entry's first HIP call.

A case is one call with at least one bad argument; the table holds the returned
status and the exact ``pdsc_last_error()`` text.  Each entry has one case per
``fail(`` site that can be reached before device work (the too-small workspace
among them: a dummy non-null ``ws`` with ``ws_bytes`` one short of the size
query; its byte counts are recorded as <size-1> and <size>, see replay), and
"precedence" cases that break two checks at once, which pin the
ORDER of the checks: swapping two checks of an entry changes which of the two
messages such a call reports.

`python tests/test_abi_errors.py --write [path/to/libpdsc.so]` records the
table; only a commit that MEANS to change a check, its status or its message
should do that.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "abi_errors", "abi_errors.json")

P = "P"          # a dummy non-null pointer (never dereferenced: the call fails first)
BIG = 1 << 40    # a workspace size that passes every need_ws


def short(query, *args):
    """ws_bytes one byte short of `query(*args)`."""
    return {"short_of": [query, list(args)]}


def cfg(**fields):
    """A pdsc_config argument: _lib.make_config()'s defaults (3 layers) with `fields` set."""
    return {"cfg": fields}


def ptrs(n, null_at):
    """An array of n dummy pointers with entry `null_at` NULL (pdsc_pack_weights' parameter list)."""
    return {"ptrs": [n, null_at]}


C0 = cfg()
ENC_WS = ("pdsc_encoder_workspace_bytes", C0, 2, 100)
ATT_WS = ("pdsc_attention_workspace_bytes", 2, 100, 128, 0)


# entry -> (a VALID argument list, [overrides breaking one check each], [overrides breaking two checks])
# An override maps argument positions to values; the valid list itself is never called.
ENTRIES = {
    # f1 (corr.hip)
    "pdsc_mutual_nn": (
        [P, P, 10, 12, 32, P, P, P, BIG, None],
        [{0: None}, {7: None}, {2: 0}, {3: 0}, {4: 0}, {4: 65}, {8: short("pdsc_mutual_nn_workspace_bytes", 10, 12)},
         {5: None}, {6: None}],
        [{0: None, 2: 0}, {4: 65, 8: short("pdsc_mutual_nn_workspace_bytes", 10, 12)},
         {8: short("pdsc_mutual_nn_workspace_bytes", 10, 12), 5: None}]),
    "pdsc_build_correspondences": (
        [P, P, P, P, 10, 12, 32, 1, None, 0.1, P, P, P, P, P, None, P, BIG, None],
        [{0: None}, {4: 0}, {6: 65}, {17: short("pdsc_mutual_nn_workspace_bytes", 10, 12)}, {2: None}, {14: None},
         {8: P}],
        [{1: None, 4: 0}, {6: 65, 17: short("pdsc_mutual_nn_workspace_bytes", 10, 12)},
         {17: short("pdsc_mutual_nn_workspace_bytes", 10, 12), 2: None}, {2: None, 8: P}]),
    # f3 (sm.hip, training.hip)
    "pdsc_spectral_matching": (
        [P, P, P, 100, 0.1, 0.1, 10, P, P, None, P, BIG, None],
        [{0: None}, {10: None}, {3: 0}, {3: 46341}, {6: -1}, {5: 1.5}, {5: "nan"}, {4: 0.0},
         {11: short("pdsc_spectral_matching_workspace_bytes", 100)}],
        [{8: None, 3: 0}, {6: -1, 11: short("pdsc_spectral_matching_workspace_bytes", 100)}]),
    "pdsc_sm_compat": (
        [P, 100, 0.1, P, None],
        [{0: None}, {3: None}, {1: 0}, {1: 46341}, {2: 0.0}, {2: "nan"}],
        [{0: None, 1: 0}, {1: 46341, 2: 0.0}]),
    "pdsc_sm_matvec": (
        [P, P, 10, P, None],
        [{0: None}, {3: None}, {2: 0}],
        [{1: None, 2: 0}]),
    "pdsc_spectral_matching_loss": (
        [P, P, 2, 100, 1, P, P, BIG, None],
        [{0: None}, {6: None}, {2: 0}, {3: 0}, {7: short("pdsc_spectral_matching_loss_workspace_bytes", 2, 100)}],
        [{5: None, 3: 0}, {2: 0, 7: short("pdsc_spectral_matching_loss_workspace_bytes", 2, 100)}]),
    # f4 (descriptors.hip)
    "pdsc_ply_read_xyz": (
        ["no/such/cloud.ply", P, 10, P],
        [{0: None}, {3: None}, {}],  # {}: the path does not exist ("PLY: cannot open ...")
        []),
    "pdsc_radius_knn": (
        [P, 100, 0.1, 30, P, None, P, P, BIG, None],
        [{0: None}, {1: 0}, {2: 0.0}, {2: "inf"}, {2: "nan"}, {3: 0}, {3: 129}, {4: None}, {6: None}, {7: None},
         {8: short("pdsc_radius_knn_workspace_bytes", 100)}],
        [{0: None, 1: 0}, {1: 0, 2: 0.0}, {2: -1.0, 3: 0}, {3: 129, 4: None},
         {4: None, 8: short("pdsc_radius_knn_workspace_bytes", 100)}]),
    "pdsc_estimate_normals": (
        [P, 100, 0.1, 30, 0, None, P, P, BIG, None],
        [{0: None}, {3: 129}, {6: None}, {4: 3}, {4: -1}, {4: 1},
         {8: short("pdsc_estimate_normals_workspace_bytes", 100, 30)}],
        [{1: 0, 6: None}, {6: None, 4: 3}, {4: 1, 8: short("pdsc_estimate_normals_workspace_bytes", 100, 30)}]),
    "pdsc_voxel_down_sample": (
        [P, None, 100, 0.05, P, None, P, P, BIG, None],
        [{0: None}, {2: 0}, {3: -1.0}, {4: None}, {6: None}, {8: short("pdsc_voxel_down_sample_workspace_bytes", 100)}],
        [{3: 0.0, 4: None}, {4: None, 8: short("pdsc_voxel_down_sample_workspace_bytes", 100)}]),
    "pdsc_compute_fpfh": (
        [P, P, 100, 0.1, 30, P, None, P, BIG, None],
        [{0: None}, {4: 129}, {1: None}, {5: None}, {8: short("pdsc_compute_fpfh_workspace_bytes", 100, 30)}],
        [{4: 129, 1: None}, {5: None, 8: short("pdsc_compute_fpfh_workspace_bytes", 100, 30)}]),
    # f5 (icp.hip)
    "pdsc_icp_point_to_point": (
        [P, 100, P, 120, None, 0.1, 30, 1e-6, 1e-6, P, P, None, P, BIG, None],
        [{1: 0}, {3: 0}, {5: 0.0}, {5: "nan"}, {5: "inf"}, {6: -1}, {0: None}, {2: None}, {12: None},
         {13: short("pdsc_icp_workspace_bytes", 100, 120)}],
        [{1: 0, 5: 0.0}, {5: 0.0, 6: -1}, {6: -1, 0: None}, {2: None, 13: short("pdsc_icp_workspace_bytes", 100, 120)}]),
    # f6 (ransac.hip)
    "pdsc_ransac_correspondence": (
        [P, P, 100, 0.1, 3, 0.9, 1000, 0.999, 1, 0, P, P, P, None, P, BIG, None],
        [{4: 5}, {4: 2}, {2: 2}, {6: 0}, {3: 0.0}, {3: "inf"}, {7: 0.0}, {7: 1.5}, {5: 1.5}, {5: -0.1}, {0: None},
         {14: None}, {15: short("pdsc_ransac_workspace_bytes", 100)}],
        [{4: 5, 2: 2}, {2: 2, 6: 0}, {6: 0, 3: 0.0}, {3: 0.0, 7: 0.0}, {7: 1.5, 5: 1.5}, {5: 1.5, 0: None},
         {1: None, 15: short("pdsc_ransac_workspace_bytes", 100)}]),
    "pdsc_refit_inliers": (
        [P, P, P, 100, 0.1, P, None, None, None, None],
        [{3: 0}, {4: 0.0}, {4: "inf"}, {0: None}, {5: None}],
        [{3: 0, 4: 0.0}, {4: "nan", 5: None}]),
    # f7 (match_filter.hip)
    "pdsc_nn2": (
        [P, P, 100, 120, 32, P, P, P, P, BIG, None],
        [{2: 0}, {3: 1}, {4: 0}, {4: 65}, {0: None}, {7: None}, {8: None}, {9: short("pdsc_nn2_workspace_bytes", 100, 120)}],
        [{3: 1, 4: 65}, {4: 65, 0: None}, {7: None, 9: short("pdsc_nn2_workspace_bytes", 100, 120)}]),
    "pdsc_nn2_split": (
        [P, P, 100, 120, 32, 2, P, P, P, P, BIG, None],
        [{5: 0}, {4: 65}, {6: None}, {10: short("pdsc_nn2_workspace_bytes", 100, 120)}],
        [{5: 0, 2: 0}, {2: 0, 0: None}, {8: None, 10: short("pdsc_nn2_workspace_bytes", 100, 120)}]),
    "pdsc_match_ratio": (
        [P, P, 100, 120, 32, P, P, P, P, P, P, P, None],
        [{2: 0}, {4: 65}, {9: None}, {8: None}, {11: None}],
        [{4: 65, 9: None}, {5: None, 10: None}]),
    "pdsc_gpf_select": (
        [P, P, P, 100, 10, 1.0, P, P, None, None, P, BIG, None],
        [{3: 0}, {4: 0}, {4: 65}, {3: 262145}, {5: -1.0}, {5: "inf"}, {0: None}, {10: None},
         {11: short("pdsc_gpf_select_workspace_bytes", 100, 10)}],
        [{3: 0, 4: 65}, {4: 65, 3: 262145}, {3: 262145, 5: -1.0}, {5: "nan", 0: None},
         {6: None, 11: short("pdsc_gpf_select_workspace_bytes", 100, 10)}]),
    # f8 (clique.hip)
    "pdsc_consistency_graph": (
        [P, 100, 0.1, 0, P, None, None],
        [{1: 0}, {1: 8193}, {2: 0.0}, {2: "inf"}, {3: 2}, {0: None}, {4: None}],
        [{1: 0, 2: 0.0}, {1: 8193, 2: 0.0}, {2: 0.0, 3: 2}, {3: -1, 4: None}]),
    "pdsc_max_clique": (
        [P, 100, 0, P, P, None, P, BIG, None],
        [{1: 0}, {1: 8193}, {2: -1}, {0: None}, {4: None}, {7: short("pdsc_max_clique_workspace_bytes", 100)}],
        [{1: 8193, 2: -1}, {2: -1, 0: None}, {3: None, 7: short("pdsc_max_clique_workspace_bytes", 100)}]),
    "pdsc_greedy_clique": (
        [P, 100, P, P, None, P, BIG, None],
        [{1: 0}, {1: 8193}, {0: None}, {6: short("pdsc_max_clique_workspace_bytes", 100)}],
        [{1: 8193, 0: None}, {3: None, 6: short("pdsc_max_clique_workspace_bytes", 100)}]),
    # f9 (teaser.hip)
    "pdsc_gnc_tls_rotation": (
        [P, P, 100, 0.1, 1.4, 100, 1e-6, P, None, None, None, None],
        [{2: 0}, {2: 8193}, {3: 0.0}, {3: "inf"}, {4: 1.0}, {4: "inf"}, {5: 0}, {6: "nan"}, {0: None}, {7: None}],
        [{2: 8193, 3: 0.0}, {3: 0.0, 4: 1.0}, {4: 1.0, 5: 0}, {5: 0, 6: "nan"}, {6: "nan", 7: None}]),
    "pdsc_tls_translation": (
        [P, P, 100, 0.1, P, None, P, BIG, None],
        [{2: 0}, {2: 8193}, {3: "inf"}, {4: None}, {6: None}, {7: short("pdsc_tls_translation_workspace_bytes", 100)}],
        [{2: 0, 3: 0.0}, {3: 0.0, 4: None}, {4: None, 7: short("pdsc_tls_translation_workspace_bytes", 100)}]),
    "pdsc_teaser_solve": (
        [P, P, 100, 0.1, 1.4, 100, 1e-6, 0, P, None, None, P, BIG, None],
        [{2: 0}, {2: 8193}, {3: 0.0}, {4: 1.0}, {5: 0}, {6: "nan"}, {7: -1}, {8: None}, {11: None},
         {12: short("pdsc_teaser_solve_workspace_bytes", 100)}],
        [{2: 8193, 3: 0.0}, {3: 0.0, 4: 0.5}, {6: "nan", 7: -1}, {7: -1, 8: None},
         {8: None, 12: short("pdsc_teaser_solve_workspace_bytes", 100)}]),
    # f10 (gc_ransac.hip)
    "pdsc_gc_grid": (
        [P, P, 100, 16, P, P, P, P, P, BIG, None],
        [{2: 0}, {2: 262145}, {3: 0}, {3: 1025}, {4: None}, {8: None}, {9: short("pdsc_gc_grid_workspace_bytes", 100)}],
        [{2: 262145, 3: 0}, {3: 1025, 4: None}, {7: None, 9: short("pdsc_gc_grid_workspace_bytes", 100)}]),
    "pdsc_gc_label": (
        [P, P, P, 100, P, P, P, 0.1, 0.5, P, P, None, P, BIG, None],
        [{3: 0}, {3: 262145}, {7: 0.0}, {7: "inf"}, {8: 1.5}, {8: "nan"}, {0: None}, {10: None}, {12: None},
         {13: short("pdsc_gc_label_workspace_bytes", 100)}],
        [{3: 0, 7: 0.0}, {7: 0.0, 8: 1.5}, {8: -0.5, 0: None}, {9: None, 13: short("pdsc_gc_label_workspace_bytes", 100)}]),
    "pdsc_gc_ransac": (
        [P, P, 100, 0.1, 0.5, 16, 1000, 0.999, 1, 1, P, P, P, None, P, BIG, None],
        [{2: 2}, {2: 262145}, {6: 0}, {3: 0.0}, {4: 1.5}, {7: 0.0}, {7: "nan"}, {5: 0}, {5: 1025}, {0: None}, {14: None},
         {15: short("pdsc_gc_ransac_workspace_bytes", 100)}],
        [{2: 2, 6: 0}, {6: 0, 3: 0.0}, {4: 1.5, 7: 0.0}, {7: 1.5, 5: 1025}, {5: 0, 0: None},
         {1: None, 15: short("pdsc_gc_ransac_workspace_bytes", 100)}]),
    # f13 (rgbd_odometry.hip): the pyramid entry, odo_check's frame checks in their order
    "pdsc_rgbd_odometry_pyramid": (
        [P, P, 2, 8, 16, 0.0, 4.0, 0, P, None, None, None, None, None, P, BIG, None],
        [{0: None}, {1: None}, {14: None}, {2: 0}, {3: 4}, {4: 4}, {3: 10}, {4: 18}, {2: 65536}, {3: 8192, 4: 8196},
         {5: -1.0}, {5: "nan"}, {6: 0.0}, {5: 4.0}, {6: "inf"}, {7: -1}, {7: 3},
         {15: short("pdsc_rgbd_odometry_workspace_bytes", 2, 8, 16, 1)}],
        [{0: None, 2: 0}, {2: 0, 3: 4}, {3: 4, 2: 65536}, {2: 65536, 6: 0.0}, {6: 0.0, 7: 3},
         {7: 3, 15: short("pdsc_rgbd_odometry_workspace_bytes", 2, 8, 16, 1)}]),
    # a1 (compat.hip)
    "pdsc_compat_f32": (
        [P, P, 2, 10, P, P, None],
        [{0: None}, {4: None}, {5: None}, {2: 0}, {3: 0}],
        [{1: None, 2: 0}, {5: None, 3: 0}]),
    "pdsc_compat_packed_f32": (
        [P, P, 2, 10, P, P, None],
        [{0: None}, {4: None}, {5: None}, {2: 0}, {3: 0}],
        [{1: None, 2: 0}, {5: None, 3: 0}]),
    # a5 (seeds.hip)
    "pdsc_pick_seeds": (
        [P, P, 2, 100, 0.1, 10, P, P, None],
        [{0: None}, {1: None}, {6: None}, {7: None}, {2: 0}, {3: 0}, {5: 0}, {5: 101}],
        [{6: None, 5: 0}, {1: None, 2: 0}]),
    # a6 (knn.hip)
    "pdsc_seed_knn": (
        [P, P, 2, 100, 128, 10, 8, 0, P, P, BIG, None],
        [{7: 2}, {7: -1}, {4: 64}, {0: None}, {1: None}, {8: None}, {9: None}, {2: 0}, {5: 0}, {6: 0}, {6: 100}, {6: 64},
         {10: short("pdsc_seed_knn_workspace_bytes", 2, 100, 10)}],
        [{7: 2, 4: 64}, {4: 64, 0: None}, {1: None, 2: 0}, {6: 64, 10: short("pdsc_seed_knn_workspace_bytes", 2, 100, 10)}]),
    # a7-a8 (nsm.hip)
    "pdsc_nsm_weights": (
        [P, P, P, P, 2, 100, 128, 10, 8, 10, 0, P, P, P, None, P, BIG, None],
        [{6: 64}, {0: None}, {1: None}, {2: None}, {3: None}, {11: None}, {12: None}, {13: None}, {15: None}, {4: 0},
         {7: 0}, {8: 0}, {8: 64}, {5: 8}, {9: -1}, {9: 32}, {10: 2},
         {16: short("pdsc_nsm_workspace_bytes", 2, 100, 10, 8, 10)}],
        [{6: 64, 0: None}, {1: None, 4: 0}, {9: 32, 10: 2},
         {10: 2, 16: short("pdsc_nsm_workspace_bytes", 2, 100, 10, 8, 10)}]),
    # a9-a11 (hypotheses.hip)
    "pdsc_rigid_transform_3d": (
        [P, P, None, 2, 10, P, None],
        [{0: None}, {1: None}, {5: None}, {3: 0}, {4: -1}],
        [{0: None, 3: 0}, {5: None, 4: -1}]),
    "pdsc_seed_hypotheses": (
        [P, P, P, P, 2, 100, 10, 8, 0.1, P, P, None, P, P, P, BIG, None],
        [{0: None}, {1: None}, {2: None}, {3: None}, {9: None}, {12: None}, {13: None}, {4: 0}, {6: 0}, {7: 0}, {7: 64},
         {5: 8}, {10: None}, {14: None}, {15: short("pdsc_seed_hypotheses_workspace_bytes", 2, 10)}],
        [{2: None, 4: 0}, {7: 64, 10: None}, {10: None, 14: None},
         {10: None, 15: short("pdsc_seed_hypotheses_workspace_bytes", 2, 10)}]),
    "pdsc_post_refine": (
        [P, P, P, 2, 100, 0.1, None],
        [{0: None}, {1: None}, {2: None}, {3: 0}, {4: 0}],
        [{1: None, 3: 0}, {0: None, 4: 0}]),
    # a2-a4: the weights (pack.hip); check_cfg's branches are reached here
    "pdsc_pack_weights": (
        [C0, P, P, None],
        [{0: None}, {0: cfg(num_channels=64)}, {0: cfg(num_layers=0)}, {0: cfg(num_layers=65)}, {0: cfg(in_dim=0)},
         {0: cfg(in_dim=129)}, {0: cfg(num_iterations=-1)}, {0: cfg(num_iterations=32)}, {0: cfg(k=0)},
         {0: cfg(precision=2)}, {1: None}, {2: None}, {1: ptrs(88, 0)}, {1: ptrs(88, 30)}, {1: ptrs(88, 87)}],
        [{0: None, 1: None}, {0: cfg(num_channels=64, num_layers=0)}, {0: cfg(num_layers=0, in_dim=0)},
         {0: cfg(in_dim=0, num_iterations=32)}, {0: cfg(num_iterations=32, k=0)}, {0: cfg(k=0, precision=2)},
         {0: cfg(precision=2), 1: None}, {2: None, 1: ptrs(88, 5)}]),
    "pdsc_packed_block": (
        [C0, 0, 0, P],
        [{0: None}, {0: cfg(in_dim=129)}, {1: -1}, {1: 3}, {2: -1}, {2: 8}, {3: None}],
        [{0: cfg(num_layers=65), 1: -1}, {1: 3, 2: 8}, {2: 8, 3: None}]),
    # a2-a4: the standalone encoder (encoder.hip); the shape checks are reached here
    "pdsc_encoder_f32": (
        [C0, P, P, P, 2, 100, None, P, P, P, BIG, None],
        [{0: None}, {0: cfg(precision=2)}, {4: 0}, {5: 1}, {5: 32768}, {5: 5}, {0: cfg(k=64)}, {0: cfg(ratio=0.001)},
         {1: None}, {2: None}, {3: None}, {7: None}, {8: None}, {9: None}, {10: short(*ENC_WS)}],
        [{0: cfg(k=0), 4: 0}, {4: 0, 5: 32768}, {5: 32768, 0: cfg(ratio=0.00001)}, {5: 5, 0: cfg(k=64)},
         {0: cfg(k=64), 1: None}, {5: 1, 1: None}, {3: None, 10: short(*ENC_WS)}]),
    # a3: the standalone attention (attention.hip)
    "pdsc_attention_f32": (
        [P, P, P, P, 2, 100, 128, 0, P, P, BIG, None],
        [{6: 64}, {0: None}, {1: None}, {2: None}, {3: None}, {8: None}, {9: None}, {4: 0}, {5: 0}, {5: 32768}, {7: 2},
         {7: -1}, {10: short(*ATT_WS)}],
        [{6: 64, 0: None}, {8: None, 4: 0}, {5: 32768, 7: 2}, {0: None, 7: 2}, {4: 0, 10: short(*ATT_WS)}]),
    # the row's timing, layout and plan queries (encoder.hip) and the forward's plan query (api.hip)
    "pdsc_attention_timing": (
        [P, P, 4, P],
        [{0: None}, {1: None}, {3: None}],
        [{0: None, 3: None}]),
    "pdsc_diag_qkv_delay": (
        [0],
        [{0: -1}],
        []),
    "pdsc_attention_layout": (
        [2, 100, 0, P, P],
        [{2: 2}, {2: -1}, {0: 0}, {1: 0}, {3: None}, {4: None}],
        [{2: 2, 0: 0}, {1: 0, 3: None}]),
    "pdsc_encoder_plan": (
        [2, 100, 0, P],
        [{2: 2}, {0: 0}, {1: 0}, {3: None}],
        [{2: 2, 3: None}, {0: 0, 1: 0}]),
    "pdsc_encoder_plan_vfold": (
        [2, 100, 0, P],
        [{2: 2}, {0: 0}, {1: 0}, {3: None}],
        [{2: 2, 3: None}, {0: 0, 1: 0}]),
    "pdsc_launch_plan": (
        [C0, 2, 100, P, 13],
        [{0: None}, {0: cfg(num_layers=0)}, {1: 0}, {2: 1}, {2: 32768}, {2: 5}, {0: cfg(k=64)}, {3: None}, {3: None, 4: 12}],
        [{0: cfg(in_dim=0), 1: 0}, {2: 32768, 0: cfg(ratio=0.00001)}, {2: 5, 0: cfg(k=64)}, {0: cfg(k=64), 3: None},
         {1: 0, 4: 12}]),
}


def cases():
    """[(entry, kind, args)] in table order; args with the overrides applied (JSON-ready)."""
    out = []
    for entry, (valid, singles, pairs) in ENTRIES.items():
        for kind, overrides in (("check", singles), ("precedence", pairs)):
            for o in overrides:
                assert kind == "check" or len(o) in (1, 2) or entry == "pdsc_ply_read_xyz", (entry, o)
                args = list(valid)
                for i, v in o.items():
                    args[i] = v
                out.append((entry, kind, args))
    return out


def bind(path=None):
    """The library's entries with their argument types (pointdsc_amd._lib's table)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from pointdsc_amd import _lib
    if path is None:
        return _lib.load(), _lib._PROTOS
    lib = ctypes.CDLL(path)
    for name, (res, argtypes) in _lib._PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, argtypes
    return lib, _lib._PROTOS


_DUMMY = ctypes.create_string_buffer(256)


def _convert(lib, v, ctype, protos=None):
    if isinstance(v, dict) and "cfg" in v:
        from pointdsc_amd import _lib
        c = _lib.make_config(num_layers=3)
        for k, x in v["cfg"].items():
            setattr(c, k, x)
        return ctypes.pointer(c)
    if isinstance(v, dict) and "ptrs" in v:
        n, null_at = v["ptrs"]
        arr = (ctypes.c_void_p * n)(*([ctypes.addressof(_DUMMY)] * n))
        arr[null_at] = None
        return arr
    if isinstance(v, dict):
        query, qargs = v["short_of"]
        size = getattr(lib, query)(*(_convert(lib, a, t) for a, t in zip(qargs, protos[query][1])))
        assert size > 0, (query, qargs)
        return size - 1
    if v == P:
        if ctype in (ctypes.c_void_p, ctypes.c_char_p):
            return ctypes.addressof(_DUMMY)
        return ctypes.cast(_DUMMY, ctype)  # a typed pointer argument
    if isinstance(v, str):
        return v.encode() if ctype is ctypes.c_char_p else float(v)  # "nan", "inf"
    return v


def replay(lib, protos):
    """[(status, message)] of cases(), in order.

    The bytes of a too-small workspace appear in the message as <size-1> and
    <size>: the sizes of the grid stages hold hipcub's temporary storage, which
    varies with the device the process sees, so the table records the text
    around the live size query's value (test_workspace_table.py pins the sizes).
    """
    got = []
    for entry, _, args in cases():
        argtypes = protos[entry][1]
        assert len(args) == len(argtypes), entry
        call = [_convert(lib, v, t, protos) for v, t in zip(args, argtypes)]
        status = getattr(lib, entry)(*call)
        msg = lib.pdsc_last_error().decode()
        for v, c in zip(args, call):
            if isinstance(v, dict) and "short_of" in v:
                msg = msg.replace(f"{c} < {c + 1} bytes", "<size-1> < <size> bytes")
        got.append((int(status), msg))
    return got


def test_every_case_is_rejected_on_the_host():
    """The recording holds only argument errors: no success, no HIP status."""
    with open(FIXTURE) as f:
        table = json.load(f)["cases"]
    assert table
    for row in table:
        assert row["status"] in (1, 3), row  # PDSC_ERR_ARG, PDSC_ERR_UNSUPPORTED
        assert row["error"], row


def test_abi_errors_match_recording():
    with open(FIXTURE) as f:
        table = json.load(f)["cases"]
    want_cases = [[e, k, a] for e, k, a in cases()]
    assert [[r["entry"], r["kind"], r["args"]] for r in table] == json.loads(json.dumps(want_cases))
    lib, protos = bind()
    bad = []
    for row, (status, msg) in zip(table, replay(lib, protos)):
        if (status, msg) != (row["status"], row["error"]):
            bad.append(f'{row["entry"]} [{row["kind"]}] args={row["args"]}: got ({status}, {msg!r}), '
                       f'recorded ({row["status"]}, {row["error"]!r})')
    assert not bad, f"{len(bad)} calls differ from the recording:\n" + "\n".join(bad)


def test_table_covers_every_moved_entry():
    """Each entry has single-check cases, the workspace one where it takes a workspace, and precedence cases."""
    _, protos = bind()
    for entry, (valid, singles, pairs) in ENTRIES.items():
        assert len(valid) == len(protos[entry][1]), entry
        assert singles, entry
        if entry not in ("pdsc_ply_read_xyz", "pdsc_diag_qkv_delay"):
            assert pairs, entry
        if ctypes.c_size_t in protos[entry][1]:
            assert any(isinstance(v, dict) and "short_of" in v for o in singles for v in o.values()), entry
            assert any(isinstance(v, dict) and "short_of" in v for o in pairs for v in o.values()), entry


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        lib, protos = bind(sys.argv[2] if len(sys.argv) > 2 else None)
        rows = [{"entry": e, "kind": k, "args": a, "status": s, "error": m}
                for (e, k, a), (s, m) in zip(cases(), replay(lib, protos))]
        hip = [r for r in rows if r["status"] not in (1, 3)]
        assert not hip, f"cases that passed the host checks: {hip}"
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        with open(FIXTURE, "w") as f:
            f.write('{"cases": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
        print("wrote", FIXTURE, len(rows), "cases")
    else:
        sys.exit("usage: test_abi_errors.py --write [libpdsc.so]")
