"""ctypes binding of libneat_hip.so (C ABI declared in include/neat_hip.h).

There is NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os

import torch

NUM_LAYERS = 19
ABI_VERSION = 15
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "fp16x3": 4}
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NEAT_HIP_LIB") or os.path.join(_HERE, "csrc", "libneat_hip.so")      # NEAT_HIP_LIB: a probe build (scripts/probes/abl_build.sh)

c_fp = ctypes.c_void_p      # device float* (passed as integer addresses)


class NetParams(ctypes.Structure):
    _fields_ = [("v", c_fp * NUM_LAYERS), ("g", c_fp * NUM_LAYERS), ("b", c_fp * NUM_LAYERS)]


class NetGrads(ctypes.Structure):
    _fields_ = [("dv", c_fp * NUM_LAYERS), ("dg", c_fp * NUM_LAYERS), ("db", c_fp * NUM_LAYERS)]


class EvalGrid(ctypes.Structure):
    """neat_eval_grid_t: a uniform cell grid over a cloud (neat_amd/evaluate.py builds it)."""
    _fields_ = [("origin", ctypes.c_double * 3), ("cell", ctypes.c_double), ("dim", ctypes.c_int * 3), ("buckets", ctypes.c_int),
                ("dense", ctypes.c_int), ("n", ctypes.c_int), ("start", c_fp), ("sidx", c_fp), ("spts", c_fp)]


_SIGNATURES = {
    "neat_abi_version": (ctypes.c_int, []),
    "neat_packed_floats": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_pack_weights": (ctypes.c_int, [ctypes.POINTER(NetParams), c_fp, ctypes.c_int, c_fp]),
    "neat_eik_points": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp, c_fp]),
    "neat_camera_rays": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_sdf_ws_floats": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "neat_sdf_forward": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_sdf_backward": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp,
                                         ctypes.POINTER(NetGrads), c_fp]),
    "neat_sdf_backward_x": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_fp, c_fp,
                                           c_fp, c_fp, ctypes.POINTER(NetGrads), c_fp, c_fp]),
    "neat_heads_ws_floats": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_heads_forward": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp,
                                          c_fp, c_fp, c_fp]),
    "neat_render_ws_floats": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "neat_render_forward": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_fp,
                                           c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp]),
    "neat_render_eval_ws_floats": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "neat_render_forward_eval": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_fp,
                                                c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_render_backward": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, c_fp, ctypes.c_float, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.POINTER(NetGrads), c_fp, c_fp,
                                            c_fp]),
    "neat_sampler_bound": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp,
                                          ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_sampler_resample": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_float,
                                             c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_sampler_finish": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_sample_pdf": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp, c_fp]),
    "neat_uniform_depths": (ctypes.c_int, [c_fp, ctypes.c_float, c_fp, ctypes.c_float, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_sdf_values_gated": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                             ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_sdf_values_rays": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_sampler_init": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int,
                                         c_fp]),
    "neat_sampler_bound_dev": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp,
                                              ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_sampler_resample_dev": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_float,
                                                 c_fp, ctypes.c_int, c_fp, c_fp, c_fp,
                                                 c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, ctypes.c_int,
                                                 c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp]),
    "neat_sampler_finish_dev": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_float,
                                               ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_sdf_ldp": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "neat_adam_step_coef": (ctypes.c_int, [c_fp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, c_fp, c_fp,
                                           c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_fp]),
    "neat_loss_lines_terms": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_float, c_fp, c_fp, ctypes.c_float,
                                             c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int,
                                             c_fp, c_fp, c_fp, c_fp, ctypes.c_float, c_fp, c_fp, c_fp, c_fp]),
    "neat_camera_setup": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_project2d_pair": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_sdf_values_laid_out": (ctypes.c_int, [c_fp, ctypes.POINTER(NetParams), ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_sampler_init_rays": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_sampler_round": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_sampler_finish_picked": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_encode_lines": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_gather_batch": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, ctypes.c_int,
                                         c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_copy_batch": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_ffn_forward": (ctypes.c_int, [c_fp, ctypes.c_int] + [c_fp] * 10),
    "neat_ffn_backward": (ctypes.c_int, [c_fp, ctypes.c_int] + [c_fp] * 15),
    "neat_l3d": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp]),
    "neat_junction_cost": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_junction_gate": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp,
                                          c_fp, c_fp, c_fp]),
    "neat_loss_terms": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int,
                                       c_fp, c_fp, c_fp, c_fp, ctypes.c_float, c_fp]),
    "neat_loss_pairs": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp,
                                       c_fp, c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_camera_mats": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_inv_small": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_project2d": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp]),
    "neat_project2d_backward": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_line_loss": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_float, c_fp, c_fp, c_fp, c_fp]),
    "neat_line_losses": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_float, c_fp, c_fp, ctypes.c_float, c_fp]),
    "neat_adam_step": (ctypes.c_int, [c_fp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int),
                                      ctypes.c_int, c_fp, c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_fp]),
    "neat_lsap_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_lsap": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_dbscan_ws_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_dbscan_means": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_double, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_parse_match": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_fp, c_fp, c_fp]),
    "neat_parse_group_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_parse_group": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_parse_vote_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_parse_vote": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_parse_graph_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "neat_parse_graph": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_fp, c_fp, c_fp, ctypes.c_int,
                                        c_fp, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_parse_visibility_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_parse_visibility": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_float,
                                             ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_grid_points": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), c_fp]),
    "neat_mesh_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "neat_mesh_count": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_fp, c_fp, c_fp]),
    "neat_mesh_emit": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double), ctypes.c_float, c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp]),
    "neat_unit_rows3": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp]),
    "neat_grid_points_affine": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
                                + [ctypes.POINTER(ctypes.c_double)] * 4 + [c_fp]),
    "neat_mesh_moments_ws_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_mesh_moments": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), c_fp, c_fp, c_fp, c_fp]),
    "neat_affine_rows3": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), c_fp]),
    "neat_affine_bounds3_ws_bytes": (ctypes.c_size_t, []),
    "neat_affine_bounds3": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), c_fp, c_fp, c_fp]),
    "neat_mesh_cut_count": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_mesh_cut_emit": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_fp, c_fp, c_fp, c_fp,
                                          ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp]),
    "neat_eval_grid_ws_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_eval_grid": (ctypes.c_int, [c_fp, ctypes.POINTER(EvalGrid), c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_eval_thin_round": (ctypes.c_int, [c_fp, ctypes.POINTER(EvalGrid), ctypes.c_double, c_fp, c_fp, c_fp]),
    "neat_eval_nearest": (ctypes.c_int, [ctypes.POINTER(EvalGrid), c_fp, ctypes.c_int, ctypes.c_double, c_fp, c_fp, c_fp]),
    "neat_eval_obs_mask": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double), ctypes.c_double, c_fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                          c_fp, c_fp]),
    "neat_eval_tri_ws_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_eval_tri_count": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_double, c_fp, c_fp, c_fp]),
    "neat_eval_tri_emit": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_double, c_fp, c_fp, ctypes.c_int, c_fp]),
    "neat_eval_line_cost": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_show_ws_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "neat_show_ws_layout": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_size_t)]),
    "neat_show_clear": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp]),
    "neat_show_mesh": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                      c_fp, c_fp]),
    "neat_show_lines": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 4 + [c_fp, c_fp]),
    "neat_show_points": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 4 + [c_fp, c_fp]),
    "neat_show_resolve": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_double), c_fp, c_fp, c_fp]),
    "neat_frame_put": (ctypes.c_int, [c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_frame_sum_ws_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "neat_frame_sum": (ctypes.c_int, [c_fp, ctypes.c_longlong, c_fp, c_fp, c_fp]),
    "neat_frame_range_ws_bytes": (ctypes.c_size_t, []),
    "neat_frame_range": (ctypes.c_int, [c_fp, ctypes.c_longlong, c_fp, c_fp, c_fp]),
    "neat_frame_grey": (ctypes.c_int, [c_fp, ctypes.c_longlong, c_fp, c_fp, c_fp]),
    "neat_frame_grid": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_trace_ws_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_trace_list_offset": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "neat_trace_init": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_double, ctypes.c_double, c_fp, c_fp, c_fp, c_fp]),
    "neat_trace_step": (ctypes.c_int, [c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                       ctypes.c_int, c_fp, c_fp, c_fp, c_fp]),
    "neat_trace_finish": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_trace_target_rays": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_double, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_raycast_bvh_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_raycast_ws_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "neat_raycast_build": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_raycast_cast": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_post_fuse_ws_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "neat_post_fuse": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, ctypes.c_int, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_post_select": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_post_refine_ws_bytes": (ctypes.c_size_t, [ctypes.c_int] * 2),
    "neat_post_refine_view": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp,
                                             ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_fp, c_fp, c_fp, c_fp]),
    "neat_post_snap_ws_bytes": (ctypes.c_size_t, [ctypes.c_int] * 2),
    "neat_post_snap": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_detect_label": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, c_fp]),
    "neat_detect_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int]),
    "neat_detect_lines": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_fp, c_fp, ctypes.c_int]
                          + [ctypes.c_double] * 6 + [ctypes.c_int, c_fp, ctypes.c_int] + [c_fp] * 7),
    "neat_tri_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "neat_tri_count": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_double,
                                      ctypes.c_double, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "neat_tri_fill": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, c_fp, ctypes.c_double, ctypes.c_double,
                                     c_fp, ctypes.c_longlong, c_fp, c_fp, c_fp, c_fp]),
    "neat_tri_lines": (ctypes.c_int, [c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_fp, ctypes.c_int, c_fp, c_fp, c_fp, c_fp, ctypes.c_longlong,
                                      c_fp, c_fp, c_fp, ctypes.c_double, ctypes.c_double, ctypes.c_int] + [c_fp] * 10),
    "neat_scenegen_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int] * 2),
    "neat_scenegen_shade": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, c_fp] + [ctypes.c_int] * 4 + [ctypes.c_double] * 3 + [c_fp] * 3),
    "neat_scenegen_edge_count": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, c_fp, c_fp]
                                 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 + [c_fp] * 3),
    "neat_scenegen_edge_fill": (ctypes.c_int, [c_fp, ctypes.c_int, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp] + [ctypes.c_int] * 3
                                + [ctypes.c_double] * 4 + [c_fp, ctypes.c_longlong] + [c_fp] * 5),
    "neat_volume_weights": (ctypes.c_int, [c_fp, c_fp, ctypes.c_int, ctypes.c_int, c_fp, c_fp, c_fp]),
    "neat_set_tuning": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "neat_prof_enable": (ctypes.c_int, [ctypes.c_int]),
    "neat_prof_collect": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


def exported_symbols():
    """Names declared in include/neat_hip.h (kept in sync by tests/test_abi.py)."""
    return sorted(_SIGNATURES)


tuning_overrides = []      # the NEAT_TUNING key=value pairs applied when the library was loaded (bench.py records them)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or neat_amd/csrc/build.sh).  neat_amd has no CPU/PyTorch fallback for the hot path.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
        # A/B switches from the environment (probe scripts; the defaults are what the tests and the bench run):
        # NEAT_TUNING="16=0,21=2" -> neat_set_tuning(16, 0), neat_set_tuning(21, 2)
        applied = []
        for kv in filter(None, os.environ.get("NEAT_TUNING", "").split(",")):
            k, v = kv.split("=")
            check(l.neat_set_tuning(int(k), int(v)), f"NEAT_TUNING {kv}")
            applied.append(kv)
        if applied:       # never silent: a stray variable changes what the tests and the bench measure
            import sys
            print(f"[neat_amd] NEAT_TUNING overrides applied: {','.join(applied)}", file=sys.stderr, flush=True)
        global tuning_overrides
        tuning_overrides = applied
    return _lib


def check(code, what):
    if code != 0:
        raise RuntimeError(f"libneat_hip: {what} failed with code {code}")


def stream():
    """The current stream of the current device, as the library's hipStream_t argument."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """A tensor's device address; NULL for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None
