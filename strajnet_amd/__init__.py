"""strajnet_amd -- MI355X-native (gfx950 / CDNA4) implementation of the STrajNet forward/backward hot path.

Drop-in call surface of the reference's two classes:
    from strajnet_amd import STrajNet, OGMFlow_loss
The math runs in hand-written HIP kernels (strajnet_amd/csrc -> libstrajnet_hip.so, C ABI in include/strajnet_hip.h).
"""
from .modules import STrajNet            # noqa: F401
from .loss import (OGMFlow_loss, WaypointGrids, OccupancyFlowTaskConfig,     # noqa: F401
                   get_pred_waypoint_logits, warpped_gt)
from .optim import Nadam, DeviceNadam, CosineDecayRestarts, CustomSchedule     # noqa: F401
from .training import train_step     # noqa: F401
from .metrics import compute_occupancy_flow_metrics, apply_sigmoid_to_occupancy_logits, OccupancyFlowMetrics     # noqa: F401
from .evaluate import Mean, OGMFlowMetrics, SceneScores, print_metrics, eval_step     # noqa: F401
from .submission import (QuantizedWaypoints, ResultDrain, quantize_waypoints, quantize_reference,     # noqa: F401
                         compress_batch, compression_pool, CompressedWaypoints, compress_waypoints, compress_reference,
                         DEFLATE_SEGMENT, FramedWaypoints, SubmissionWriter, SUBMISSION_SCHEMA, frame_reference,
                         submission_reference, parse_submission)
from .data import (ResidentPool, ResidentFeed, PoolLayout, PoolWriter, PoolSampler, ShuffleWindow, WindowFeed)     # noqa: F401
from .raster import (RasterConfig, Tracks, Rasterizer, rasterize, raster_reference, raster_example,     # noqa: F401
                     tracks_from_motion_example)
