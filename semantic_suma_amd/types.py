"""ctypes mirrors of include/suma_types.h (the POD types that cross the C-ABI)."""
from __future__ import annotations

import ctypes as C

import numpy as np

u32, i32, f32, f64 = C.c_uint32, C.c_int32, C.c_float, C.c_double

WEIGHT_NONE, WEIGHT_HUBER, WEIGHT_TUKEY, WEIGHT_STABILITY = 0, 1, 2, 3
MAP_VERTEX, MAP_NORMAL, MAP_SEMANTIC = 0, 1, 2
FRAME_OLD, FRAME_NEW, FRAME_COMPOSED = 0, 1, 2
ACC_WORDS = 32
FILTER_SAMPLING_GL_INITIAL, FILTER_SAMPLING_NEAREST = 0, 1
ACC_SCALE = 268435456.0

# numpy view of the 64-byte surfel record (reference src/core/Surfel.h:5-15)
SURFEL_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("radius", "<f4"),
    ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("confidence", "<f4"),
    ("timestamp", "<u4"), ("color", "<f4"), ("weight", "<f4"), ("count", "<f4"),
    ("r", "<f4"), ("g", "<f4"), ("b", "<f4"), ("w", "<f4"),
])
assert SURFEL_DTYPE.itemsize == 64


class SumaParams(C.Structure):
    """Flattened rv::ParameterList -- field order identical to ``struct suma_params``."""
    _fields_ = [
        ("data_width", u32), ("data_height", u32), ("data_fov_up", f32), ("data_fov_down", f32),
        ("min_depth", f32), ("max_depth", f32),
        ("model_width", u32), ("model_height", u32), ("model_fov_up", f32), ("model_fov_down", f32),
        ("model_min_depth", f32), ("model_max_depth", f32),
        ("max_iterations", u32), ("stopping_threshold", f32), ("delta", f32),
        ("icp_max_distance", f32), ("icp_max_angle", f32), ("weight_function", i32), ("factor", f32),
        ("bilinear_sampling", i32),
        ("initialize_identity", i32), ("fallback_mode", i32), ("fallback_max_distance", f32),
        ("fallback_max_angle", f32),
        ("compose_rendering", i32), ("max_loop_closure_distance", f32),
        ("min_radius", f32), ("max_radius", f32), ("max_angle", f32), ("map_max_distance", f32),
        ("map_max_angle", f32), ("unstable_age", i32), ("confidence_mode", i32), ("confidence_threshold", f32),
        ("p_stable", f32), ("p_prior", f32), ("sigma_angle", f32), ("sigma_distance", f32),
        ("use_stability", i32), ("active_timestamps", i32), ("max_weight", f32), ("weighting_scheme", i32),
        ("averaging_scheme", i32), ("update_always", i32),
        ("submap_dimension", i32), ("submap_extent", f32), ("partial_extraction", i32),
        ("max_surfels", u32), ("max_poses", u32),
        ("label_offset", u32), ("prob_offset", u32), ("cache_surfels", u32),
        ("avg_vertexmap", i32), ("filter_vertexmap", i32), ("use_filtered_vertexmap", i32),
        ("bilateral_sigma_space", f32), ("bilateral_sigma_range", f32), ("filter_sampling", i32),
    ]


SEM_MAX_CLASSES = 32  # SUMA_SEM_MAX_CLASSES
SEM_CHANNELS = 5      # SUMA_SEM_CHANNELS: range, x, y, z, remission


class SemanticParams(C.Structure):
    """``struct suma_semantic_params``: geometry and normalisation of a segmentation network's range image, its class
    count and label map (the semantic front end, semantic_suma_amd/segmentation.py)."""
    _fields_ = [
        ("width", u32), ("height", u32), ("fov_up", f32), ("fov_down", f32),
        ("means", f32 * SEM_CHANNELS), ("stds", f32 * SEM_CHANNELS),
        ("n_classes", u32), ("label_map", i32 * SEM_MAX_CLASSES),
    ]


class SemanticKnnParams(C.Structure):
    """``struct suma_semantic_knn``: RangeNet++'s KNN post-processing of the back-projection (window ``search`` x
    ``search``, ``k`` voters, Gaussian ``sigma``, range ``cutoff``; segmentation.semantic_knn)."""
    _fields_ = [("search", u32), ("k", u32), ("sigma", f32), ("cutoff", f32)]


DRAW_MAX_LIGHTS = 10   # SUMA_DRAW_MAX_LIGHTS
DRAW_MAX_SIZE = 8192   # SUMA_DRAW_MAX_SIZE: width and height
DRAW_COLORS = 260      # SUMA_DRAW_COLORS: texels of the semantic colour map


class DrawLight(C.Structure):
    """``struct suma_draw_light``: one light of draw_surfels.geom (position.w < 0.0001: directional)"""
    _fields_ = [("position", f32 * 4), ("ambient", f32 * 3), ("diffuse", f32 * 3), ("specular", f32 * 3)]


class DrawParams(C.Structure):
    """``struct suma_draw_params``: camera, viewport and the uniforms of SurfelMap::draw (core.SurfelMap.draw)"""
    _fields_ = [
        ("mvp", f32 * 16), ("view_pos", f32 * 3), ("width", u32), ("height", u32), ("color_mode", i32),
        ("conf_threshold", f32), ("backface_culling", i32), ("use_stability", i32), ("clear_color", f32 * 4),
        ("num_lights", u32), ("lights", DrawLight * DRAW_MAX_LIGHTS),
        ("mat_ambient", f32 * 3), ("mat_diffuse", f32 * 3), ("mat_specular", f32 * 3), ("mat_emission", f32 * 3),
        ("mat_shininess", f32), ("mat_alpha", f32), ("color_map", (C.c_uint8 * 3) * DRAW_COLORS),
    ]


# numpy view of the 48-byte world-frame record (``struct suma_world_surfel``, SurfelMap.export_world)
WORLD_SURFEL_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("radius", "<f4"),
    ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("confidence", "<f4"),
    ("label", "<u4"), ("prob", "<f4"), ("timestamp", "<u4"), ("support", "<u4"),
])
assert WORLD_SURFEL_DTYPE.itemsize == 48


class WorldParams(C.Structure):
    """``struct suma_world_params``: voxel size (0: one record per surfel), confidence and label filters of
    SurfelMap.export_world; ``WorldParams.defaults()`` = suma_world_params_default"""
    _fields_ = [("voxel_size", f32), ("min_confidence", f32), ("keep_label", C.c_uint8 * DRAW_COLORS)]

    @classmethod
    def defaults(cls, voxel_size: float = 0.0, min_confidence=None, keep_labels=None) -> "WorldParams":
        """``keep_labels``: None (all), or the label ids to keep"""
        p = cls(voxel_size=voxel_size, min_confidence=float("-inf") if min_confidence is None else min_confidence)
        keep = set(range(DRAW_COLORS)) if keep_labels is None else {int(l) for l in keep_labels}
        for l in range(DRAW_COLORS):
            p.keep_label[l] = 1 if l in keep else 0
        return p


class WorldStats(C.Structure):
    """``struct suma_world_stats``: what one export read, filtered, dropped and produced"""
    _fields_ = [("n_active", u32), ("n_tiles", u32), ("n_parked", u32), ("n_passed", u32), ("n_dropped", u32),
                ("n_out", u32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# numpy view of the 48-byte cell of the traversability grid (``struct suma_grid_cell``, core.world_grid)
GRID_CELL_DTYPE = np.dtype([
    ("ground_z", "<f4"), ("ground_rough", "<f4"), ("z_min", "<f4"), ("z_max", "<f4"),
    ("obstacle_z", "<f4"), ("prob", "<f4"), ("label", "<u4"), ("support", "<u4"),
    ("n_ground", "<u4"), ("n_obstacle", "<u4"), ("n_overhang", "<u4"),
    ("state", "u1"), ("ground_source", "u1"), ("pad", "u1", (2,)),
])
assert GRID_CELL_DTYPE.itemsize == 48
GRID_UNKNOWN, GRID_FREE, GRID_OBSTACLE, GRID_NO_GROUND = 0, 1, 2, 3
GRID_GROUND_LABELS = (40, 44, 48, 49, 60, 72)  # road, parking, sidewalk, other-ground, lane-marking, terrain


class GridParams(C.Structure):
    """``struct suma_grid_params``: the raster (cell size, origin, width x height) and the rules of core.world_grid;
    ``GridParams.defaults()`` = suma_grid_params_default"""
    _fields_ = [("cell_size", f32), ("origin_x", f32), ("origin_y", f32), ("width", u32), ("height", u32),
                ("ground_label", C.c_uint8 * DRAW_COLORS), ("min_normal_z", f32), ("step_height", f32),
                ("clearance", f32), ("fill_radius", u32)]

    @classmethod
    def defaults(cls, cell_size: float = 0.2, origin=(0.0, 0.0), width: int = 0, height: int = 0, ground_labels=None,
                 min_normal_z: float = 0.7, step_height: float = 0.2, clearance: float = 2.0,
                 fill_radius: int = 2) -> "GridParams":
        """``ground_labels``: None (GRID_GROUND_LABELS), or the label ids that count as ground; width = height = 0: to
        be fitted (core.world_grid does so)"""
        p = cls(cell_size=cell_size, origin_x=origin[0], origin_y=origin[1], width=width, height=height,
                min_normal_z=min_normal_z, step_height=step_height, clearance=clearance, fill_radius=fill_radius)
        for l in (GRID_GROUND_LABELS if ground_labels is None else ground_labels):
            p.ground_label[int(l)] = 1
        return p

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "ground_label"}
        d["ground_labels"] = [l for l in range(DRAW_COLORS) if self.ground_label[l]]
        return d


class GridStats(C.Structure):
    """``struct suma_grid_stats``: records dropped / outside / binned, cells by state"""
    _fields_ = [("n_records", u32), ("n_dropped", u32), ("n_outside", u32), ("n_binned", u32), ("n_occupied", u32),
                ("n_free", u32), ("n_obstacle", u32), ("n_no_ground", u32), ("n_filled", u32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# numpy view of the 8-byte cell of the planner's field (``struct suma_plan_cell``, core.grid_plan)
PLAN_CELL_DTYPE = np.dtype([("cost", "<u4"), ("clear2", "<u2"), ("flags", "u1"), ("next", "u1")])
assert PLAN_CELL_DTYPE.itemsize == 8
# the result for one start of core.grid_paths (``struct suma_plan_path``)
PLAN_PATH_DTYPE = np.dtype([("length", "<u4"), ("status", "<u4"), ("cost", "<u4"), ("pad", "<u4")])
PLAN_UNREACHED = 0xffffffff
PLAN_MAX_CLEAR_CELLS, PLAN_MAX_GOALS, PLAN_MAX_STARTS = 64, 4096, 4096
# direction k of a move as (dx, dy): E, NE, N, NW, W, SW, S, SE; the row index grows with y
PLAN_DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
PLAN_AT_GOAL, PLAN_NO_DIRECTION = 8, 255
PLAN_BLOCKED, PLAN_TRAVERSABLE, PLAN_REACHED = 1, 2, 4  # bits of the cell's flags
PATH_OK, PATH_UNREACHED, PATH_START_OUTSIDE, PATH_TRUNCATED, PATH_BAD_FIELD = 0, 1, 2, 3, 4
PATH_STATUS_NAMES = ("OK", "UNREACHED", "START_OUTSIDE", "TRUNCATED", "BAD_FIELD")


class PlanParams(C.Structure):
    """``struct suma_plan_params``: the robot (radius, step, roughness), the clearance window and the costs of
    core.grid_plan; ``PlanParams.defaults()`` = suma_plan_params_default"""
    _fields_ = [("robot_radius", f32), ("max_step", f32), ("max_rough", f32), ("unknown_blocked", u32),
                ("max_clear_cells", u32), ("soft_cells", u32), ("soft_weight", u32), ("label_cost", C.c_uint8 * DRAW_COLORS)]

    @classmethod
    def defaults(cls, robot_radius: float = 0.4, max_step: float = 0.15, max_rough: float = float("nan"),
                 unknown_blocked: bool = True, max_clear_cells: int = 16, soft_cells: int = 3, soft_weight: int = 2,
                 label_cost=None) -> "PlanParams":
        """``label_cost``: None (all 1), a dict label -> cost over a base of 1, or 260 values; 0 = forbidden"""
        p = cls(robot_radius=robot_radius, max_step=max_step, max_rough=max_rough, unknown_blocked=int(bool(unknown_blocked)),
                max_clear_cells=max_clear_cells, soft_cells=soft_cells, soft_weight=soft_weight)
        cost = [1] * DRAW_COLORS
        if isinstance(label_cost, dict):
            for l, v in label_cost.items():
                cost[int(l)] = int(v)
        elif label_cost is not None:
            cost = [int(v) for v in label_cost]
            if len(cost) != DRAW_COLORS:
                raise ValueError(f"label_cost: {len(cost)} values, {DRAW_COLORS} wanted")
        for l in range(DRAW_COLORS):
            p.label_cost[l] = cost[l]
        return p

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "label_cost"}
        d["label_cost"] = {l: self.label_cost[l] for l in range(DRAW_COLORS) if self.label_cost[l] != 1}
        return d


class PlanStats(C.Structure):
    """``struct suma_plan_stats``: cells blocked / traversable / reached, goals given / ignored, the largest cost, rounds"""
    _fields_ = [("n_blocked", u32), ("n_traversable", u32), ("n_reached", u32), ("n_goals", u32), ("n_goals_ignored", u32),
                ("max_cost", u32), ("n_rounds", u32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# SurfelMap's constructor (SurfelMap.cpp:195-229): the value each uniform of draw_surfels_ is left with.  Only light 0
# is used (num_lights = 1); lights 1-4 are the "evenly distributed sun light" it also sets.
DRAW_LIGHTS = [
    dict(position=(0.0, -1.0, -1.0, 0.0), ambient=(0.4, 0.4, 0.4), diffuse=(0.6, 0.52944, 0.4566), specular=(0.3, 0.3, 0.3)),
] + [dict(position=d, ambient=(0.1,) * 3, diffuse=(0.1,) * 3, specular=(0.1,) * 3)
     for d in ((1, -1, 1, 0), (-1, -1, 1, 0), (1, -1, -1, 0), (-1, -1, -1, 0))]
DRAW_MATERIAL = dict(ambient=(0.75, 0.65, 0.5), diffuse=(1.0, 0.9, 0.7), specular=(1.0, 1.0, 1.0),
                     emission=(0.0, 0.0, 0.0), shininess=16.0, alpha=1.0)


class IcpStats(C.Structure):
    _fields_ = [("error", f64), ("inlier_residual", f64), ("valid", u32), ("outlier", u32), ("inlier", u32),
                ("invalid", u32), ("iterations", u32), ("converged", u32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LocalizerParams(C.Structure):
    """``struct suma_localizer_params``: render threshold, the two gates and the motion model of core.Localizer;
    ``LocalizerParams.defaults(params)`` = suma_localizer_params_default"""
    _fields_ = [("conf_threshold", f32), ("min_valid_ratio", f32), ("max_outlier_ratio", f32),
                ("constant_velocity", i32)]

    @classmethod
    def defaults(cls, params: "SumaParams" = None, **overrides) -> "LocalizerParams":
        p = cls(conf_threshold=0.0 if params is None else params.confidence_threshold, min_valid_ratio=0.2,
                max_outlier_ratio=0.85, constant_velocity=1)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(f"unknown parameter {k!r}")
            setattr(p, k, v)
        return p


class LocalizerResult(C.Structure):
    """``struct suma_localizer_result``: what one localised scan gave (matrices column-major, as the C-ABI has them;
    core.Localizer.processScan hands them out row-major)"""
    _fields_ = [("guess", f64 * 16), ("pose", f64 * 16), ("increment", f64 * 16), ("stats", IcpStats),
                ("valid_ratio", f32), ("outlier_ratio", f32), ("tracked", i32), ("window_rebuilt", i32),
                ("origin_ij", i32 * 2), ("n_window", u32)]


class ChangeParams(C.Structure):
    """``struct suma_change_params``: what counts as seen through, grazing and too far for the change evidence of
    core.Localizer (csrc/k_change.hip); ``ChangeParams.defaults()`` = suma_change_params_default"""
    _fields_ = [("free_margin", f32), ("min_view_cos", f32), ("max_range", f32), ("tracked_only", i32)]

    @classmethod
    def defaults(cls, **overrides) -> "ChangeParams":
        p = cls(free_margin=0.5, min_view_cos=0.3, max_range=50.0, tracked_only=1)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(f"unknown parameter {k!r}")
            setattr(p, k, v)
        return p


class ChangeCounts(C.Structure):
    """``struct suma_change_counts``: what one observation did with the records of the window"""
    _fields_ = [("n_window", u32), ("unseen", u32), ("no_return", u32), ("occluded", u32), ("misses", u32),
                ("grazing", u32), ("hits", u32), ("near", u32), ("label_changes", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ChangeRule(C.Structure):
    """``struct suma_change_rule``: a record is removed iff misses >= min_misses and misses > miss_ratio * hits (fp32);
    ``ChangeRule.defaults()`` = suma_change_rule_default"""
    _fields_ = [("min_misses", u32), ("miss_ratio", f32)]

    @classmethod
    def defaults(cls, min_misses: int = 3, miss_ratio: float = 2.0) -> "ChangeRule":
        return cls(min_misses=min_misses, miss_ratio=miss_ratio)


# numpy view of ``struct suma_change_evidence``: one per record of the map, in the map's record order
EVIDENCE_DTYPE = np.dtype([("hits", "<u4"), ("misses", "<u4"), ("occluded", "<u4"), ("label_changes", "<u4")])
assert EVIDENCE_DTYPE.itemsize == 16


class NovelParams(C.Structure):
    """``struct suma_novel_params``: what the collection of newly seen surfaces of core.Localizer (csrc/k_novel.hip) takes
    for explained and too far, and how many candidates it holds; ``NovelParams.defaults()`` = suma_novel_params_default"""
    _fields_ = [("agree_margin", f32), ("max_range", f32), ("tracked_only", i32), ("max_candidates", u32)]

    @classmethod
    def defaults(cls, **overrides) -> "NovelParams":
        p = cls(agree_margin=0.5, max_range=50.0, tracked_only=1, max_candidates=4194304)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


DESKEW_TIME_AZIMUTH, DESKEW_TIME_TIMES = 0, 1
DESKEW_MOTION_NONE, DESKEW_MOTION_INCREMENT, DESKEW_MOTION_OVERRIDE = 0, 1, 2


class DeskewParams(C.Structure):
    """``struct suma_deskew_params``: how the motion compensation of raw sweeps (csrc/k_deskew.hip) times a point and
    which instant of the sweep it refers to; ``DeskewParams.defaults()`` = suma_deskew_params_default"""
    _fields_ = [("time_source", i32), ("clockwise", i32), ("start_azimuth", f32), ("t_ref", f32), ("scale", f32)]

    @classmethod
    def defaults(cls, **overrides) -> "DeskewParams":
        p = cls(time_source=DESKEW_TIME_AZIMUTH, clockwise=0, start_azimuth=0.0, t_ref=0.5, scale=1.0)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class NovelFuseParams(C.Structure):
    """``struct suma_novel_fuse_params``; ``NovelFuseParams.defaults(params)`` = suma_novel_fuse_params_default: the
    confidence new records get is confidence_threshold + 1, so that the localiser renders them"""
    _fields_ = [("voxel_size", f32), ("min_views", u32), ("confidence", f32)]

    @classmethod
    def defaults(cls, params=None, **overrides) -> "NovelFuseParams":
        conf = C.c_float((params.confidence_threshold if params is not None else 0.0)).value
        p = cls(voxel_size=0.2, min_views=2, confidence=float(np.float32(conf) + np.float32(1.0)))
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class NovelCounts(C.Structure):
    """``struct suma_novel_counts``: what one collection did with the texels of the frame"""
    _fields_ = [("n_texels", u32), ("no_return", u32), ("out_of_range", u32), ("grazing", u32), ("explained", u32),
                ("novel", u32), ("stored", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


NOVEL_COUNTS = tuple(k for k, _ in NovelCounts._fields_)


class NovelStats(C.Structure):
    """``struct suma_novel_stats``"""
    _fields_ = [("n_candidates", u32), ("n_overflow", u32), ("n_dropped", u32), ("n_voxels", u32), ("n_out", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ObjectParams(C.Structure):
    """``struct suma_object_params``: when neighbouring unexplained texels of a scan belong to one object
    (csrc/k_objects.hip) and how many objects a segmentation keeps; ``ObjectParams.defaults()`` =
    suma_object_params_default"""
    _fields_ = [("link_base", f32), ("link_slope", f32), ("min_texels", u32), ("max_objects", u32)]

    @classmethod
    def defaults(cls, **overrides) -> "ObjectParams":
        p = cls(link_base=0.3, link_slope=0.03, min_texels=5, max_objects=4096)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class ObjectCounts(C.Structure):
    """``struct suma_object_counts``: what one segmentation made of the texels of the frame"""
    _fields_ = [("n_texels", u32), ("n_members", u32), ("n_components", u32), ("n_small", u32), ("n_objects", u32),
                ("stored", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


OBJECT_COUNTS = tuple(k for k, _ in ObjectCounts._fields_)

# numpy view of ``struct suma_scan_object``: one per object of a scan, in ascending root order
SCAN_OBJECT_DTYPE = np.dtype([("root", "<u4"), ("n_texels", "<u4"), ("label", "<u4"), ("prob", "<f4"), ("n_dynamic", "<u4"),
                              ("min", "<f4", (3,)), ("max", "<f4", (3,)), ("centroid", "<f4", (3,)), ("r_min", "<f4"),
                              ("scan_id", "<u4")])
assert SCAN_OBJECT_DTYPE.itemsize == 64


class LiveParams(C.Structure):
    """``struct suma_live_params``: how long a hit keeps a cell of the live obstacle layer an obstacle, how many hits in
    a row it takes, and how far a scan's rays clear cells (csrc/k_live.hip); ``LiveParams.defaults()`` =
    suma_live_params_default"""
    _fields_ = [("hold_scans", u32), ("min_hits", u32), ("carve_range", f32), ("carve_margin", f32)]

    @classmethod
    def defaults(cls, **overrides) -> "LiveParams":
        p = cls(hold_scans=10, min_hits=2, carve_range=20.0, carve_margin=0.5)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class LiveCounts(C.Structure):
    """``struct suma_live_counts``: what one update of the live layer made of the texels of the frame"""
    _fields_ = [("n_texels", u32), ("n_members", u32), ("n_outside", u32), ("n_no_ground", u32), ("n_low", u32),
                ("n_high", u32), ("n_hit_texels", u32), ("n_hit_cells", u32), ("n_rays", u32), ("n_cleared", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class LiveStats(C.Structure):
    """``struct suma_live_stats``: the cells with a hit by what a compose made of them"""
    _fields_ = [("n_live", u32), ("n_pending", u32), ("n_expired", u32), ("n_carved", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


LIVE_COUNTS = tuple(k for k, _ in LiveCounts._fields_)
LIVE_STATS = tuple(k for k, _ in LiveStats._fields_)
# numpy view of ``struct suma_live_cell``: the raw state of one cell of the live layer
LIVE_CELL_DTYPE = np.dtype([("hit", "<u8"), ("clear", "<u4"), ("hits", "<u4")])
assert LIVE_CELL_DTYPE.itemsize == 16
LIVE_MASK_LIVE, LIVE_MASK_PENDING = 1, 2


class TrackParams(C.Structure):
    """``struct suma_track_params``: when the objects of a scan are fragments of one thing, how near a detection must
    be to a track's prediction, the gains of the filter, and when a track is confirmed and dropped
    (csrc/k_tracks.hip); ``TrackParams.defaults()`` = suma_track_params_default"""
    _fields_ = [("join_dist", f32), ("gate_base", f32), ("gate_speed", f32), ("alpha", f32), ("beta", f32),
                ("confirm_hits", u32), ("max_missed", u32), ("max_tracks", u32), ("max_rounds", u32)]

    @classmethod
    def defaults(cls, **overrides) -> "TrackParams":
        p = cls(join_dist=2.0, gate_base=1.5, gate_speed=0.5, alpha=0.5, beta=0.2, confirm_hits=3, max_missed=3,
                max_tracks=1024, max_rounds=16)
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class TrackCounts(C.Structure):
    """``struct suma_track_counts``: what one update of the tracks made of the objects of a scan"""
    _fields_ = [("n_objects", u32), ("n_detections", u32), ("n_joined", u32), ("n_tracks_before", u32), ("n_matched", u32),
                ("n_missed", u32), ("n_expired", u32), ("n_born", u32), ("n_dropped", u32), ("n_confirmed", u32),
                ("n_unresolved", u32), ("rounds", u32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


TRACK_COUNTS = tuple(k for k, _ in TrackCounts._fields_)
# numpy view of ``struct suma_object_track``: one slot of the tracker's table
OBJECT_TRACK_DTYPE = np.dtype([("id", "<u4"), ("slot", "<u4"), ("state", "<u4"), ("label", "<u4"), ("n_texels", "<u4"),
                               ("n_dynamic", "<u4"), ("n_objects", "<u4"), ("hits", "<u4"), ("missed", "<u4"),
                               ("first_stamp", "<u4"), ("last_matched", "<u4"), ("position", "<f4", (3,)),
                               ("velocity", "<f4", (3,)), ("origin", "<f4", (3,)), ("min", "<f4", (3,)), ("max", "<f4", (3,)),
                               ("r_min", "<f4"), ("detection", "<u4")])
assert OBJECT_TRACK_DTYPE.itemsize == 112
TRACK_FREE, TRACK_TENTATIVE, TRACK_CONFIRMED, TRACK_NO_DETECTION = 0, 1, 2, 0xffffffff


class ObjectTrack:
    """one record of OBJECT_TRACK_DTYPE with what a consumer asks of it"""

    def __init__(self, record):
        self.record = record
        for k in OBJECT_TRACK_DTYPE.names:
            v = record[k]
            setattr(self, k, v.copy() if isinstance(v, np.ndarray) else (float(v) if k == "r_min" else int(v)))

    @property
    def confirmed(self) -> bool:
        return self.state == TRACK_CONFIRMED

    @property
    def age(self) -> int:
        """scan-id steps between the founding and the last match"""
        return self.last_matched - self.first_stamp

    @property
    def net_velocity(self) -> np.ndarray:
        """(position - origin) / age in metres per scan-id step: the average over the track's life, zero at age 0"""
        d = (self.position.astype(np.float64) - self.origin.astype(np.float64))
        return d / self.age if self.age else np.zeros(3)

    def as_dict(self):
        return dict(id=self.id, slot=self.slot, confirmed=self.confirmed, label=self.label, n_texels=self.n_texels,
                    n_objects=self.n_objects, hits=self.hits, missed=self.missed, first_stamp=self.first_stamp,
                    last_matched=self.last_matched, position=[float(x) for x in self.position],
                    velocity=[float(x) for x in self.velocity], net_velocity=[float(x) for x in self.net_velocity],
                    age=self.age, detection=self.detection)


PLACE_MAX_DIM = 64       # SUMA_PLACE_MAX_DIM: rings and sectors
PLACE_MAX_MATCHES = 32   # SUMA_PLACE_MAX_MATCHES
# is_dynamic_label (csrc/dev_math.h): the moving classes K1 drops at the start of a run
DYNAMIC_LABELS = (10, 11, 13, 15, 18, 20, 30, 31, 32)


class PlaceParams(C.Structure):
    """``struct suma_place_params``: geometry and label mask of a place descriptor (core.PlaceIndex);
    ``PlaceParams.defaults()`` = suma_place_params_default"""
    _fields_ = [("rings", u32), ("sectors", u32), ("max_range", f32), ("height_offset", f32),
                ("keep_label", C.c_uint8 * DRAW_COLORS)]

    @classmethod
    def defaults(cls, keep_labels=None, **overrides) -> "PlaceParams":
        """``keep_labels``: None (all), or the label ids to keep"""
        p = cls(rings=20, sectors=60, max_range=80.0, height_offset=2.0)
        keep = set(range(DRAW_COLORS)) if keep_labels is None else {int(l) for l in keep_labels}
        for l in range(DRAW_COLORS):
            p.keep_label[l] = 1 if l in keep else 0
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(f"unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @classmethod
    def static_only(cls, **overrides) -> "PlaceParams":
        """the defaults without the moving classes (is_dynamic_label)"""
        return cls.defaults(keep_labels=set(range(DRAW_COLORS)) - set(DYNAMIC_LABELS), **overrides)


class PlaceMatch(C.Structure):
    """``struct suma_place_match``: one candidate place of a query"""
    _fields_ = [("index", u32), ("id", u32), ("distance", f32), ("shift", i32), ("yaw", f32)]

    def as_dict(self):
        return dict(index=int(self.index), id=int(self.id), distance=float(self.distance), shift=int(self.shift),
                    yaw=float(self.yaw))


class RelocalizeCandidate(C.Structure):
    """``struct suma_relocalize_candidate``"""
    _fields_ = [("match", PlaceMatch), ("reserved", i32), ("result", LocalizerResult)]


class RelocalizeResult(C.Structure):
    """``struct suma_relocalize_result``: what core.Localizer.relocalize found and every candidate it tried"""
    _fields_ = [("found", i32), ("n_tried", u32), ("winner", i32), ("reserved", i32), ("match", PlaceMatch),
                ("reserved2", i32), ("result", LocalizerResult), ("candidates", RelocalizeCandidate * PLACE_MAX_MATCHES)]


def default_params(**overrides) -> SumaParams:
    """Values of the reference's config/default.xml (same as suma_params_default in suma_types.h)."""
    p = SumaParams(
        data_width=900, data_height=64, data_fov_up=3.0, data_fov_down=-25.0, min_depth=2.0, max_depth=75.0,
        model_width=900, model_height=64, model_fov_up=3.0, model_fov_down=-25.0, model_min_depth=2.0,
        model_max_depth=75.0,
        max_iterations=33, stopping_threshold=1e-4, delta=1e-4,
        icp_max_distance=2.0, icp_max_angle=30.0, weight_function=WEIGHT_HUBER, factor=0.5, bilinear_sampling=1,
        initialize_identity=0, fallback_mode=1, fallback_max_distance=0.5, fallback_max_angle=30.0,
        compose_rendering=1, max_loop_closure_distance=8.0,
        min_radius=0.03, max_radius=1.0, max_angle=90.0, map_max_distance=0.2, map_max_angle=45.0,
        unstable_age=3, confidence_mode=3, confidence_threshold=0.0, p_stable=0.6, p_prior=0.5,
        sigma_angle=1.0, sigma_distance=1.0, use_stability=1, active_timestamps=100, max_weight=20.0,
        weighting_scheme=0, averaging_scheme=0, update_always=0,
        submap_dimension=4, submap_extent=10.0, partial_extraction=1,
        max_surfels=2048 * 2048, max_poses=10000, label_offset=4, prob_offset=5, cache_surfels=0,
        avg_vertexmap=0, filter_vertexmap=0, use_filtered_vertexmap=0, bilateral_sigma_space=0.0,
        bilateral_sigma_range=2.5, filter_sampling=FILTER_SAMPLING_GL_INITIAL,
    )
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise KeyError(f"unknown parameter {k!r}")
        setattr(p, k, v)
    return p


def params_with_size(width: int, height: int = 64, **overrides) -> SumaParams:
    """default.xml with data and model images of ``width x height`` (BASELINE configs use 64x900 / 64x2048)."""
    return default_params(data_width=width, data_height=height, model_width=width, model_height=height, **overrides)


class PosegraphParams(C.Structure):
    """suma_posegraph_params (include/suma_hip.h); ``PosegraphParams.defaults()`` = gtsam's LevenbergMarquardtParams"""
    _fields_ = [("lambda_initial", f64), ("lambda_factor", f64), ("lambda_upper_bound", f64),
                ("lambda_lower_bound", f64), ("min_model_fidelity", f64), ("relative_error_tol", f64),
                ("absolute_error_tol", f64), ("error_tol", f64), ("cg_tolerance", f64),
                ("cg_max_iterations", u32), ("reserved", u32)]

    @classmethod
    def defaults(cls, **overrides) -> "PosegraphParams":
        p = cls(lambda_initial=1e-5, lambda_factor=10.0, lambda_upper_bound=1e5, lambda_lower_bound=0.0,
                min_model_fidelity=1e-3, relative_error_tol=1e-5, absolute_error_tol=1e-5, error_tol=0.0,
                cg_tolerance=1e-10, cg_max_iterations=1000)
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


PG_MAX_ITERATIONS, PG_CONVERGED, PG_LAMBDA_BOUND, PG_ERROR_TOL = 0, 1, 2, 3


class PosegraphStats(C.Structure):
    """suma_posegraph_stats (include/suma_hip.h)"""
    _fields_ = [("iterations", u32), ("termination", u32), ("cg_iterations", u32), ("linear_solves", u32),
                ("lambda_", f64), ("initial_error", f64), ("final_error", f64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LoopParams(C.Structure):
    """suma_loop_params (include/suma_hip.h); ``LoopParams.defaults()`` = suma_loop_params_default: the reference's
    values (SurfelMapping.h:221-228), the literal gates of checkLoopClosure, identity information"""
    _fields_ = [("residual_threshold", f32), ("outlier_threshold", f32), ("valid_threshold", f32),
                ("search_distance", f32), ("min_trajectory_distance", f32), ("min_verifications", i32),
                ("delta_timestamp", i32), ("optimize_wait", i32), ("min_valid_ratio", f64), ("max_outlier_ratio", f64),
                ("max_increment_difference", f64), ("information", f64 * 36), ("optimize_iterations", u32),
                ("integrate_lag", u32), ("node_capacity", u32), ("reserved", u32)]

    @classmethod
    def defaults(cls, **overrides) -> "LoopParams":
        p = cls(residual_threshold=1.05, outlier_threshold=1.1, valid_threshold=0.9, search_distance=20.0,
                min_trajectory_distance=200.0, min_verifications=3, delta_timestamp=100, optimize_wait=1,
                min_valid_ratio=0.2, max_outlier_ratio=0.85, max_increment_difference=0.1, optimize_iterations=100,
                integrate_lag=0, node_capacity=1024)
        for k in range(6):
            p.information[7 * k] = 1.0
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise KeyError(f"unknown parameter {k!r}")
            setattr(p, k, v)
        return p


class LoopStatus(C.Structure):
    """suma_loop_status (include/suma_hip.h): what one scan's loop closing did"""
    _fields_ = [("found_candidate", i32), ("use_candidate", i32), ("candidate_to", i32), ("n_unverified", u32),
                ("already_verified", i32), ("loop_count", i32), ("time_without_loop_closure", u32),
                ("currently_optimizing", i32), ("started_optimization", i32), ("integrated", i32), ("edges_added", u32),
                ("result_old_outlier_ratio", f32), ("result_old", IcpStats), ("result_old_residual", f64),
                ("loop_valid_ratio", f32), ("loop_outlier_ratio", f32), ("loop_relative_error_all", f32),
                ("reserved", f32), ("posegraph_error", f64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("result_old", "reserved")}
        d["result_old"] = self.result_old.as_dict()
        return d


CHECKPOINT_VERSION = 1        # SUMA_CHECKPOINT_VERSION
CHECKPOINT_MAX_SECTIONS = 16  # SUMA_CHECKPOINT_MAX_SECTIONS


class CheckpointSection(C.Structure):
    """``struct suma_checkpoint_section``: one directory entry as suma_checkpoint_info reports it"""
    _fields_ = [("id", u32), ("reserved", u32), ("bytes", C.c_uint64), ("digest", C.c_uint64)]


class CheckpointInfo(C.Structure):
    """``struct suma_checkpoint_info``: what a checkpoint image holds (core.checkpoint_info)"""
    _fields_ = [("version", u32), ("timestamp", u32), ("n_active", u32), ("n_tiles", u32), ("n_parked", C.c_uint64),
                ("n_nodes", u32), ("n_edges", u32), ("has_loop", i32), ("has_opt", i32), ("n_sections", u32),
                ("reserved", u32), ("total_bytes", C.c_uint64), ("sections", CheckpointSection * CHECKPOINT_MAX_SECTIONS)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("sections", "reserved")}
        d["sections"] = [dict(id=s.id, bytes=s.bytes, digest=s.digest) for s in self.sections[:self.n_sections]]
        return d
