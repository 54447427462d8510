"""ctypes binding of libsemdepth.so (include/semdepth.h).  No compute happens in Python.

The library is built in-tree by ``semantic_depth_amd.build`` / ``__graft_entry__.build()``.  If it is
missing this module raises: there is no CPU or PyTorch fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsemdepth.so")

SD_OK = 0
SD_ERR_INVALID, SD_ERR_HIP, SD_ERR_STATE, SD_ERR_NOTFOUND, SD_ERR_FORMAT = -1, -2, -3, -4, -5
SD_ENC_VGG, SD_ENC_RESNET50 = 0, 1
SD_NET_FCN8S, SD_NET_MONODEPTH = 0, 1
SD_PLY_ROW_CAP, SD_PLY_HEADER_CAP, SD_PLY_LINE_ROWS = 69, 209, 1001
# the segments of a scene file (sd_scene_format's mask), in file order
(SD_SCENE_ROAD, SD_SCENE_ROAD_PLANE, SD_SCENE_RW_LINE, SD_SCENE_FENCE_L, SD_SCENE_FENCE_R, SD_SCENE_PLANE_L, SD_SCENE_PLANE_R,
 SD_SCENE_F2F_LINE) = (1 << i for i in range(8))
SD_SCENE_ALL = 255
SD_TEXT_MAX_BYTES, SD_TEXT_MAX_SEGS, SD_TEXT_MAX_ITEMS, SD_TEXT_MAX_SCALE_Q8, SD_TEXT_MAX_THICKNESS, SD_TEXT_MAX_ORG = 64, 32, 4, 4096, 32, 32768
SD_RENDER_MAX_EXTENT, SD_RENDER_MAX_POINT = 16384, 16
SD_PROFILE_MAX_DEPTHS = 256
SD_OVERLAY_MAX_SEGS, SD_OVERLAY_MAX_COORD, SD_OVERLAY_MAX_THICKNESS = 4 * 256 + 2, 32768, 32
SD_SEG_CELLS = 10      # sd_seg_confusion: counters per frame, the 3 x 3 matrix and the predictions above 2
SD_CMAP_GRAY, SD_CMAP_PLASMA = 0, 1      # sd_disp_image: the two colour maps
SD_PREC_F32, SD_PREC_BF16X2, SD_PREC_MIXED, SD_PREC_PLAN, SD_PREC_BF16X3, SD_PREC_F16X2 = 0, 1, 2, 3, 4, 5


class sd_camera(C.Structure):
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("f", C.c_double), ("b", C.c_double), ("disp_mult", C.c_double)]


class sd_rw_params(C.Structure):
    _fields_ = [("depth", C.c_double), ("z_cut", C.c_double), ("mad_y", C.c_double), ("mad_x", C.c_double),
                ("plane_thr", C.c_double), ("sor_k", C.c_int32), ("sor_ratio", C.c_double), ("ror_n", C.c_int32),
                ("ror_r", C.c_double), ("window", C.c_double), ("depth_offset", C.c_double), ("use_o3d", C.c_int32)]


class sd_rw_result(C.Structure):
    _fields_ = [("width", C.c_double), ("x_left", C.c_float), ("x_right", C.c_float), ("left_pt", C.c_float * 3),
                ("right_pt", C.c_float * 3), ("found", C.c_int32), ("n_road", C.c_int32), ("n_zcut", C.c_int32),
                ("n_mad_y", C.c_int32), ("n_mad_x", C.c_int32), ("n_plane", C.c_int32), ("n_sor", C.c_int32),
                ("n_ror", C.c_int32), ("plane", C.c_double * 4)]


class sd_text_item(C.Structure):
    _fields_ = [("text", C.c_uint8 * 64), ("len", C.c_int32), ("org_x", C.c_int32), ("org_y", C.c_int32), ("scale_q8", C.c_int32),
                ("thickness", C.c_int32), ("bgr", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class sd_render_camera(C.Structure):
    _fields_ = [("ext", C.c_double * 12), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("z_near", C.c_double), ("width", C.c_int32), ("height", C.c_int32), ("point_size", C.c_int32),
                ("background", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class sd_f2f_params(C.Structure):
    _fields_ = [("depth", C.c_double), ("mad_y", C.c_double), ("z_max", C.c_double), ("mad_left", C.c_double),
                ("mad_right", C.c_double), ("plane_thr", C.c_double)]


class sd_f2f_result(C.Structure):
    _fields_ = [("dist", C.c_double), ("left_pt", C.c_double * 3), ("right_pt", C.c_double * 3), ("plane_left", C.c_double * 4),
                ("plane_right", C.c_double * 4), ("counts", C.c_int32 * 7), ("ok", C.c_int32)]


class sd_rw_depth_result(C.Structure):
    _fields_ = [("width", C.c_double), ("x_left", C.c_float), ("x_right", C.c_float), ("left_pt", C.c_float * 3),
                ("right_pt", C.c_float * 3), ("found", C.c_int32), ("n_window", C.c_int32)]


class sd_f2f_depth_result(C.Structure):
    _fields_ = [("dist", C.c_double), ("left_pt", C.c_double * 3), ("right_pt", C.c_double * 3), ("ok", C.c_int32), ("reserved", C.c_int32)]


class sd_overlay_style(C.Structure):
    _fields_ = [("rw_bgr", C.c_uint8 * 3), ("f2f_bgr", C.c_uint8 * 3), ("edge_bgr", C.c_uint8 * 3), ("reserved", C.c_uint8 * 3),
                ("thickness", C.c_int32), ("profile_thickness", C.c_int32), ("clip_top", C.c_int32)]


class sd_overlay_segment(C.Structure):
    _fields_ = [("ax", C.c_int32), ("ay", C.c_int32), ("bx", C.c_int32), ("by", C.c_int32), ("bgr", C.c_uint8 * 3), ("thickness", C.c_uint8)]


class sd_profile_bucket(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class sd_jpeg_frame_desc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("orientation", C.c_int32), ("adobe_transform", C.c_int32), ("reserved", C.c_int32), ("blocks_w", C.c_int32 * 3),
                ("blocks_h", C.c_int32 * 3), ("coef_offset", C.c_int64 * 3), ("qt", (C.c_uint16 * 64) * 3)]

    def coef_elems(self) -> int:
        """int16 elements of the frame's coefficient buffer"""
        return sum(self.blocks_w[i] * self.blocks_h[i] * 64 for i in range(self.ncomp))

    def oriented_size(self) -> tuple:
        """(height, width) after the EXIF orientation"""
        return (self.width, self.height) if self.orientation >= 5 else (self.height, self.width)


class sd_png_frame_desc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("color_type", C.c_int32),
                ("palette_entries", C.c_int32), ("reserved", C.c_int32), ("palette", (C.c_uint8 * 3) * 256)]

    def rows_bytes(self) -> int:
        """bytes of the frame's filtered rows: a filter byte plus width * channels bytes per row"""
        return self.height * (1 + self.width * self.channels)


SD_JPEG_ENTROPY_TABLES = 8


class sd_jpeg_huff_table(C.Structure):
    _fields_ = [("look", C.c_uint16 * 512), ("mincode", C.c_int32 * 17), ("maxcode", C.c_int32 * 18), ("valptr", C.c_int32 * 17),
                ("vals", C.c_uint8 * 256)]


class sd_jpeg_entropy_frame(C.Structure):
    _fields_ = [("eligible", C.c_int32), ("ncomp", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("restart_interval", C.c_int32),
                ("n_intervals", C.c_int32), ("comp_h", C.c_int32 * 3), ("comp_v", C.c_int32 * 3), ("comp_dc", C.c_int32 * 3),
                ("comp_ac", C.c_int32 * 3), ("scan_begin", C.c_uint32), ("scan_end", C.c_uint32)]


class sd_jpeg_interval(C.Structure):
    _fields_ = [("begin", C.c_uint32), ("end", C.c_uint32)]


class sd_jpeg_sync_frame(C.Structure):
    _fields_ = [("eligible", C.c_int32), ("ncomp", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("restart_interval", C.c_int32),
                ("n_intervals", C.c_int32), ("comp_h", C.c_int32 * 3), ("comp_v", C.c_int32 * 3), ("comp_dc", C.c_int32 * 3),
                ("comp_ac", C.c_int32 * 3), ("scan_begin", C.c_uint32), ("scan_end", C.c_uint32), ("clean_bytes", C.c_uint32),
                ("subseq_bytes", C.c_uint32), ("n_pieces", C.c_uint32), ("reserved", C.c_uint32)]


class sd_jpeg_sync_interval(C.Structure):
    _fields_ = [("begin", C.c_uint32), ("end", C.c_uint32), ("first_piece", C.c_uint32), ("reserved", C.c_uint32)]


SD_JPEG_SYNC_NOT_SYNCHRONISED, SD_JPEG_SYNC_BITS_RAN_OUT, SD_JPEG_SYNC_GROUP = 5, 6, 256

# every symbol include/semdepth.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_H = C.c_void_p
SIGNATURES = {
    "sd_version": (C.c_char_p, []),
    "sd_status_string": (C.c_char_p, [C.c_int]),
    "sd_create": (C.c_int, [C.POINTER(_H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sd_create_with_plan": (C.c_int, [C.POINTER(_H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]),
    "sd_default_plan": (C.c_char_p, [C.c_int]),
    "sd_precision_plan": (C.c_int, [_H, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]),
    "sd_destroy": (C.c_int, [_H]),
    "sd_last_error": (C.c_char_p, [_H]),
    "sd_query_memory": (C.c_int, [_H, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sd_bind_memory": (C.c_int, [_H, _P, _P, _P]),
    "sd_weight_count": (C.c_int, [_H, C.c_int]),
    "sd_weight_info": (C.c_int, [_H, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "sd_load_weight": (C.c_int, [_H, C.c_int, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "sd_fcn8s_forward": (C.c_int, [_H, _P, C.c_int, _P, _P, _P, _P, _P]),
    "sd_monodepth_forward": (C.c_int, [_H, _P, C.c_int, _P, _P, _P]),
    "sd_png_unfilter_bgr": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "sd_png_decode_bgr": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sd_jpeg_decode_bgr": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sd_image_decode_bgr": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sd_decode_files_bgr": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.c_int, C.POINTER(C.c_int)]),
    "sd_jpeg_decode_coefficients": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(sd_jpeg_frame_desc)]),
    "sd_jpeg_reconstruct_bgr_host": (C.c_int, [_P, C.POINTER(sd_jpeg_frame_desc), _P, C.c_size_t]),
    "sd_decode_files_jpeg_coef": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(sd_jpeg_frame_desc),
                                            C.c_int, C.POINTER(C.c_int)]),
    "sd_jpeg_reconstruct_workspace": (C.c_int, [C.POINTER(sd_jpeg_frame_desc), C.c_int, C.POINTER(C.c_size_t)]),
    "sd_jpeg_reconstruct_bgr": (C.c_int, [_H, _P, C.c_size_t, C.POINTER(sd_jpeg_frame_desc), C.c_int, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "sd_jpeg_entropy_plan": (C.c_int, [_P, C.c_size_t, C.POINTER(sd_jpeg_frame_desc), C.POINTER(sd_jpeg_entropy_frame), _P, _P, C.c_size_t]),
    "sd_plan_files_jpeg_entropy": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t, C.c_int,
                                             C.POINTER(C.c_int)]),
    "sd_jpeg_entropy_decode_host": (C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, C.c_int, _P, C.c_size_t, _P]),
    "sd_jpeg_entropy_workspace": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sd_jpeg_entropy_decode": (C.c_int, [_H, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, C.c_int, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "sd_jpeg_sync_plan": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(sd_jpeg_frame_desc), C.POINTER(sd_jpeg_sync_frame), _P, _P, C.c_size_t, _P,
                                    C.c_size_t]),
    "sd_plan_files_jpeg_sync": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t,
                                          C.c_int, C.POINTER(C.c_int)]),
    "sd_jpeg_sync_decode_host": (C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "sd_jpeg_sync_workspace": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sd_jpeg_sync_decode": (C.c_int, [_H, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "sd_png_inflate_rows": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(sd_png_frame_desc)]),
    "sd_inflate_files_png": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(sd_png_frame_desc), C.c_int,
                                       C.POINTER(C.c_int)]),
    "sd_png_reconstruct_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    "sd_png_reconstruct_bgr": (C.c_int, [_H, _P, C.c_size_t, C.POINTER(sd_png_frame_desc), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P,
                                         C.c_size_t, _P]),
    "sd_png_encode_bgr_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.c_int, C.c_int,
                                          C.POINTER(C.c_int)]),
    "sd_png_encode_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sd_png_encode_bgr": (C.c_int, [_H, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "sd_jpeg_encode_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sd_jpeg_encode_bgr": (C.c_int, [_H, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P]),
    "sd_jpeg_encode_bgr_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sd_png_encode_zlib_host": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sd_png_write_streams_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, C.c_int,
                                             C.POINTER(C.c_int)]),
    "sd_ply_format_rows": (C.c_int64, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int]),
    "sd_ply_format_workspace": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sd_ply_format_rw": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, _P]),
    "sd_ply_format_rw_host": (C.c_int, [_P, _P, C.c_int, C.POINTER(sd_rw_result), _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "sd_text_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sd_text_draw_rw": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, _P, C.c_char_p, _P, C.c_size_t, _P]),
    "sd_text_items_rw_host": (C.c_int, [C.POINTER(sd_rw_result), C.c_char_p, C.c_int, C.c_int, C.POINTER(sd_text_item), C.POINTER(C.c_int)]),
    "sd_text_draw_host": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(sd_text_item), C.c_int]),
    "sd_text_glyph": (C.c_int, [C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sd_overlay_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sd_overlay_draw": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(sd_camera), _P, _P, _P, _P, C.c_int,
                                  C.POINTER(sd_overlay_style), _P, _P, C.c_size_t, _P]),
    "sd_overlay_segments_host": (C.c_int, [C.POINTER(sd_rw_result), _P, _P, _P, C.c_int, C.POINTER(sd_camera), C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(sd_overlay_style), C.POINTER(sd_overlay_segment), C.POINTER(C.c_int), C.POINTER(C.c_int32)]),
    "sd_overlay_draw_host": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(sd_overlay_segment), C.c_int, C.c_int]),
    "sd_render_workspace": (C.c_int, [C.c_int, C.c_int, C.POINTER(sd_render_camera), C.POINTER(C.c_size_t)]),
    "sd_render_rw": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(sd_render_camera), _P, _P, _P, C.c_size_t, _P]),
    "sd_render_rw_host": (C.c_int, [_P, _P, C.c_int, C.POINTER(sd_rw_result), C.POINTER(sd_render_camera), _P, C.POINTER(C.c_int32)]),
    "sd_post_process": (C.c_int, [_H, _P, C.c_int, _P, _P]),
    "sd_resize_cubic_u8": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P]),
    "sd_compose_result_frames": (C.c_int, [_H, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "sd_fuse_backproject": (C.c_int, [_H, _P, _P, _P, _P, C.POINTER(sd_camera), C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_postprocess_fuse_backproject": (C.c_int, [_H, _P, _P, _P, _P, _P, C.POINTER(sd_camera), C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "sd_fuse_sweep_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sd_fuse_backproject_sweep": (C.c_int, [_H, _P, _P, _P, _P, C.POINTER(sd_camera), C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                            C.c_size_t, _P]),
    "sd_road_width": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, C.POINTER(sd_rw_params), _P, _P, _P, _P, _P]),
    "sd_fence_to_fence": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(sd_f2f_params), _P, _P, _P, _P, _P, _P]),
    "sd_road_width_boxes": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, C.POINTER(sd_rw_params), _P, _P, _P, _P, _P, _P]),
    "sd_fence_to_fence_boxes": (C.c_int, [_H, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(sd_f2f_params), _P, _P, _P, _P, _P, _P, _P]),
    "sd_scene_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sd_scene_format": (C.c_int, [_H, _P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_size_t,
                                  _P, _P, _P, C.c_size_t, _P]),
    "sd_scene_format_host": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_size_t,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "sd_scene_lattice_host": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P, C.c_size_t]),
    "sd_rw_profile_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sd_road_width_profile": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_double, C.c_double, _P, _P, C.c_size_t, _P]),
    "sd_road_width_profile_host": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, _P]),
    "sd_f2f_profile": (C.c_int, [_H, _P, _P, C.c_int, _P, C.c_int, _P, _P]),
    "sd_f2f_profile_host": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "sd_resize_pil_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "sd_resize_pil_bilinear_u8": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "sd_resize_pil_bilinear_u8_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "sd_seg_confusion": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "sd_seg_confusion_host": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "sd_disp_image_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "sd_disp_image": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "sd_disp_image_host": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "sd_disp_colormap": (C.c_int, [C.c_int, _P]),
    "sd_pcl_extract_pcls": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sd_pcl_remove_from_to": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P]),
    "sd_pcl_remove_noise_by_mad": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P, _P]),
    "sd_pcl_remove_noise_by_fitting_plane": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P, _P]),
    "sd_pcl_threshold_complete": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P]),
    "sd_pcl_get_end_points_of_road": (C.c_int, [_H, _P, C.c_int, C.c_double, C.c_double, _P, _P]),
    "sd_o3d_statistical_outlier_removal": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P, _P]),
    "sd_o3d_radius_outlier_removal": (C.c_int, [_H, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P]),
    "sd_net_tensor": (C.c_int, [_H, C.c_int, C.c_char_p, _P, C.c_size_t, C.POINTER(C.c_int64), _P]),
    "sd_profile": (C.c_int, [_H, C.c_int]),
    "sd_profile_read": (C.c_int, [_H, C.POINTER(sd_profile_bucket), C.c_int, C.POINTER(C.c_int)]),
    "sd_net_flops_per_image": (C.c_double, [_H, C.c_int]),
    "sd_pass_frames": (C.c_int, [_H]),
    "sd_saturation_count": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_int]),
    "sd_saturation_count_async": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "sd_saturation_frames": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sd_saturation_settle": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "sd_set_reserved_cus": (C.c_int, [_H, C.c_int]),
    "sd_set_small_batch": (C.c_int, [_H, C.c_int]),
    "sd_small_batch_split": (C.c_int, [C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "sd_small_batch_split_direct": (C.c_int, [C.c_long, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "sd_small_batch_plan": (C.c_int, [_H, C.c_int, C.c_char_p, C.c_size_t]),
    "sd_conv_forms": (C.c_int, [_H, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
}

_lib = None


def load():
    """dlopen libsemdepth.so (after torch, so that it binds to the HIP runtime torch already loaded)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library has not been built (run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `python -m semantic_depth_amd.build`).  There is no CPU fallback for this path.")
    import torch  # noqa: F401  (loads torch/lib/libamdhip64.so, SONAME libamdhip64.so.7, which libsemdepth then shares)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if os.environ.get("SEMDEPTH_SKIP_HASH_CHECK") != "1":
        from .build import source_hash
        built, want = lib.sd_version().decode().rpartition("src=")[2], source_hash()
        if built != want:
            raise RuntimeError(f"{LIB_PATH} was built from other sources (library src={built}, tree src={want}): rebuild it with "
                               "`python -m semantic_depth_amd.build` — a stale binary is never used silently")
    _lib = lib
    return lib


class SdError(RuntimeError):
    pass


def check(lib, handle, status, what=""):
    if status != SD_OK:
        msg = lib.sd_last_error(handle).decode() if handle else ""
        raise SdError(f"{what}: {lib.sd_status_string(status).decode()} ({status}) {msg}")


def conv_launches(label, slices) -> list:
    """the kernel labels of a listed layer's launches: the reduce launch of a split layer follows its GEMM / direct launch"""
    return [label] if slices == 1 else [label, "splitk_reduce_kernel" if label.startswith("conv_splitk") else "splitc_reduce_kernel"]


def conv_forms(lib, handle, net, frames=0) -> dict:
    """{conv layer: (label, slices)} from sd_conv_forms (frames = 0: a full pass); a layer nothing can run carries its error text as the label"""
    buf = C.create_string_buffer(1 << 16)
    check(lib, handle, lib.sd_conv_forms(handle, net, frames, buf, len(buf)), "sd_conv_forms")
    out = {}
    for line in buf.value.decode().splitlines():
        name, rest = line.split(" ", 1)
        label, slices = rest.rsplit(" ", 1)
        out[name] = (label, int(slices))
    return out
