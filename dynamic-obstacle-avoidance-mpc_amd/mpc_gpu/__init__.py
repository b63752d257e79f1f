"""mpc_gpu: MI355X-native batched RTI-NMPC for the Dynamic-Obstacle-Avoidance-MPC hot path.

Host-side mirror of the reference's interface for that path; all arithmetic runs in hand-written HIP kernels behind the
C ABI of include/mpc_gpu.h (libmpcgpu.so).  There is no CPU fallback.
"""
from . import _lib
from ._lib import MpcConfig, MpcError, build, default_config
from .solver import BatchedMpc, pack_instance_bounds, pack_obstacle_mask, unpack_obstacle_mask
from .api import solve, get_solver
from .world import Obstacle, generate_random_moving_obstacles, obstacle_states
from .acados_shim import AcadosOcpSolverShim, AcadosSimSolverShim
from .closed_loop import RobotOcpProblem
from .episodes import refill_schedule, ring_model, run_episodes, run_seed_sweep, sweep_record, trace_bytes, visualisation_inputs, write_experiment
from .experiments import run_grid
from .multistart import MultiStartMpc, check_guess_geometry, group_record_bytes, multistart_record, run_multistart_episodes, run_multistart_sweep

__all__ = ["MpcConfig", "MpcError", "build", "default_config", "BatchedMpc", "pack_obstacle_mask", "unpack_obstacle_mask", "pack_instance_bounds", "solve", "get_solver", "Obstacle",
           "generate_random_moving_obstacles", "obstacle_states", "AcadosOcpSolverShim", "AcadosSimSolverShim",
           "RobotOcpProblem", "run_episodes", "run_seed_sweep", "refill_schedule", "ring_model", "sweep_record", "trace_bytes", "visualisation_inputs", "write_experiment", "run_grid", "MultiStartMpc",
           "run_multistart_episodes", "run_multistart_sweep", "check_guess_geometry", "group_record_bytes", "multistart_record"]
