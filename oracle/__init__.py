"""CPU oracle of the rollout hot path -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this package (see oracle/oracle.cpp header).  The rollout path is pinned to the
reference's own code compiled with library stand-ins (ref_py.py).
"""
from .oracle_py import (OracleResult, load, tick, samples, generate, velocity_iterator, radius_count, feed, path_blocked,  # noqa: F401
                        MarkingOracle, in_lidar_observation)
