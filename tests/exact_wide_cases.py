"""The cases of filter_bound_cases.py's coherently rounded data for the exact pass beyond 128 dimensions (test_gpu_exact_wide.py, f):
(metric, d, W, mid seed depth, seed of the assignment), chosen on the CPU with filter_bound_cases.report -- the first assignment
seed of 3 .. 7 and the smallest depth of 4 .. 15 at which the preconditions hold, which test_exact_wide_cpu.py asserts without a GPU.
numpy only."""
import filter_bound_cases as fb

BOUND_CASES = [(fb.IP, 136, 128, 8, 4), (fb.L2, 136, 1024, 7, 3), (fb.IP, 200, 128, 4, 3), (fb.L2, 200, 1024, 6, 3)]
# the floors of the existing suite: queries in which the fp32 constant loses a neighbour at the tight seed; wrong results at the mid seed
LOST_FLOOR, WRONG_FLOOR = 128, 32
