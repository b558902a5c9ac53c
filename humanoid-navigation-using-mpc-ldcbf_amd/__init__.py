"""lipmpc — MI355X-native batched LIP-MPC / LDCBF step solver (drop-in for the per-timestep MPC
solve of salvatore373/Humanoid-Navigation-using-MPC-LDCBF, HumanoidNavigation/MPC)."""
from .solver import (BatchedLipMpc, LipMpcParams, pack_rings, unpack_active, FLAG_INTERIOR, FLAG_WARM_START, FLAG_NO_PRESOLVE,  # noqa: F401
                     STATUS_SOLVED, STATUS_MAX_ITER, STATUS_INFEASIBLE, STATUS_DEGENERATE, STATUS_UNCERTIFIED,
                     STATUS_SENSOR_OVERFLOW)
from .compat import HumanoidMPC, HumanoidMPCCustomLCBF, HumanoidMPCWithRRT  # noqa: F401
from .lidar import GridMap, LidarSensor, HumanoidMPCUnknownEnvironment, UnknownEnvFleet, ray_table  # noqa: F401
from .neighbours import NeighbourRows  # noqa: F401
from .mapping import OccupancyMapper, ScanMatcher  # noqa: F401
from .planner import (RrtStarPlanner, GridFieldPlanner, FrontierPlanner, CoordinatedFrontierPlanner, InformedFrontierPlanner, TiledCoordinatedFrontierPlanner, TiledInformedFrontierPlanner, GainKeepFrontierPlanner, TiledGainKeepFrontierPlanner, RobotFieldsFrontierPlanner, FIELD_INF, RRT_FOUND, RRT_NO_PATH, RRT_START_OCCUPIED, RRT_GOAL_OCCUPIED,  # noqa: F401
                      RRT_GRID_TOO_LARGE, RRT_NO_OBSTACLE_GRID, RRT_PATH_OVERFLOW, RRT_OUTSIDE_GRID, RRT_FIELD_UNSETTLED, RRT_STATUS_NAMES, tiled_info, frontier_regions, regions_outputs)
