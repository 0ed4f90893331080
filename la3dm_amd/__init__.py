"""la3dm_amd — MI355X-native (gfx950) implementation of la3dm's per-scan occupancy-inference
hot path behind the reference's BGKOctoMap interface.  See DESIGN.md / INTEGRATION.md."""
from .bgkoctomap import BGKOctoMap, GPOctoMap, BGKLVOctoMap, BGKLOctoMap, PackedScan, FREE, OCCUPIED, UNKNOWN, PRUNED  # noqa: F401
from .bgkoctomap import MISSING, RAY_HIT, RAY_TRUNCATED, RAY_INVALID, DF_FAR, FR_MAX_CELLS, DIFF_PAIRS_CHANGED  # noqa: F401
from .bgkoctomap import GAIN_MAX_CELLS, GAIN_MAX_RAYS, GAIN_MAX_WORDS  # noqa: F401
from .bgkoctomap import SCORE_MAX_CELLS, SCORE_MAX_POINTS, SCORE_MAX_POSES, SCORE_MAX_PAIRS, SCORE_MAX_RADIUS, poses_xyz_yaw  # noqa: F401
from .bgkoctomap import SCORE_HIT, SCORE_NEAR, SCORE_FAR, SCORE_OUTSIDE, SCORE_INVALID  # noqa: F401
from .bgkoctomap import PATH_BLOCKED, PATH_LEFT, PATH_TRUNCATED, PATH_INVALID, PATH_NONE  # noqa: F401
from .bgkoctomap import PATHS_MAX_STEPS, PATHS_MAX_WAY, PATHS_MAX_PATHS, PATHS_MAX_WAYPOINTS  # noqa: F401
from .bgkoctomap import NEAREST_NONE, NEAREST_MAX_RADIUS  # noqa: F401
from .bgkoctomap import FOOTING_MAX_CELLS, FOOTING_MAX_HEADROOM, FOOTING_MAX_RADIUS, FOOTING_MAX_STEP, footprint_cells  # noqa: F401
from .bgkoctomap import SURFACE_MAX_CELLS, SURFACE_MAX_SMOOTH, surface_quads  # noqa: F401
from .bgkoctomap import REACH_NONE, REACH_MAX_CELLS, REACH_MAX_STEPS, REACH_MAX_SEEDS, REACH_BATCH  # noqa: F401
from .bgkoctomap import TRAVEL_NONE, TRAVEL_MAX_CELLS, TRAVEL_MAX_COST, TRAVEL_MAX_MOVE, TRAVEL_MAX_PENALTY, TRAVEL_MAX_SEEDS  # noqa: F401
from .bgkoctomap import TRAVEL_MAX_ROUNDS, TRAVEL_BRICK, TRAVEL_INNER, TRAVEL_BATCH, follow_parents  # noqa: F401
from .bgkoctomap import DRIVE_NONE, DRIVE_MAX_CELLS, DRIVE_MAX_MEMBERS, DRIVE_MAX_SEEDS, DRIVE_MAX_ROUNDS, DRIVE_MAX_STEP, DRIVE_MAX_SNAP  # noqa: F401
from .bgkoctomap import DRIVE_BRICK, DRIVE_INNER, DRIVE_BATCH, DRIVE_SEED_CODE, follow_drive_parents  # noqa: F401
from .bgkoctomap import CLUSTERS_NONE, CLUSTERS_MAX_CELLS, CLUSTERS_MAX_MEMBERS, CLUSTERS_MAX_ROUNDS, CLUSTERS_MAX_AXIS  # noqa: F401
from .bgkoctomap import CLUSTERS_MAX_TILE, CLUSTERS_BRICK, CLUSTERS_INNER, CLUSTERS_BATCH  # noqa: F401
from .bgkoctomap import pack_info, load_map, PACK_CLASSES  # noqa: F401
from .pcd import load_pcd  # noqa: F401
from .synth import synthetic_scan  # noqa: F401

BGK_YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=0.2, free_thresh=0.3, occupied_thresh=0.7,
                var_thresh=100.0, prior_A=0.001, prior_B=0.001)  # config/methods/bgkoctomap.yaml
GP_YAML = dict(resolution=0.1, block_depth=3, sf2=1.0, ell=1.0, noise=0.01, l=100.0, min_var=0.001, max_var=1000.0,
               max_known_var=0.02, free_thresh=0.3, occupied_thresh=0.7)  # config/methods/gpoctomap.yaml
LV_YAML = dict(resolution=0.1, block_depth=5, sf2=0.1, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=0.2,
               prior_A=0.001, prior_B=0.001, original_size=True, min_W=0.001)  # config/methods/bgklvoctomap.yaml
L_YAML = dict(resolution=0.1, block_depth=3, sf2=0.1, ell=0.2, free_thresh=0.3, occupied_thresh=0.7, var_thresh=0.15,
              prior_A=0.001, prior_B=0.001)  # config/methods/bgkloctomap.yaml (free_resolution 0.3, ds_resolution 0.1)
