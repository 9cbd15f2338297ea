"""Environment switches of the package, in two groups (README.md lists them):

PRODUCT      honoured always: they choose between supported paths of the product.
TEST HOOKS   two ranks on one GPU, gradients over gloo, ...: honoured only under NEF_TEST_HOOKS=1 (parallel._hook).

The HIP library reads no environment variable.
"""
import os

PRODUCT = {
    "NEF_H2": "1 (default): K = 1 / 3 / 7 convolutions on the split-fp16 kernels; 0: the fp32 Winograd / direct kernels (strict fp32, "
              "required for data whose dynamic range exceeds ops.H2_HEADROOM per step)",
    "NEF_H2_TAIL": "warn (default): split-fp16 call sites whose operand is heavy-tailed (ops.H2_TAIL_FRAC) are counted and reported; "
                   "fp32: such WEIGHT-GRADIENT sites run on the fp32 kernels for their lifetime (per site, per rank)",
    "NEF_H2_ALLOW_CLAMP": "1: Solver warns instead of raising when a split-fp16 launch clamped outside a protected train step",
    "NEF_LIVE": "1 (default): the encoder-side convs skip the tiles in a beat's all-zero tail (ops.LIVE / ops.LIVE_WGRAD); fwd: forward and "
                "backward-data convs only, the weight gradients multiply every item; 0: off",
    "NEF_WINOGRAD": "fp32 path: 4 (default) F(4,.) forms where allowed, 2 / 1: F(2,.) only, 0: direct kernels only",
    "NEF_SIDE_STREAM": "auto (default) / 1 / 0: weight gradients on a second HIP stream",
    "NEF_SOLVER_GRAPH": "0: Solver never replays the captured step",
    "NEF_GRAPH_SPLIT": "0: data-parallel graphed step as ONE graph + one exposed all-reduce (default: two graphs, early bucket between them)",
    "NEF_EARLY_REDUCE": "0: eager data-parallel step reduces one bucket at the optimiser step (default: early bucket under the encoder's backward)",
    "NEF_BENCH_DUMP": "bench.py: file for the per-launch event times of the breakdown steps",
    "NEF_TIE_LOG": "tests: file for the tie ratios of the decision-replaying tests",
    "NEF_TEST_HOOKS": "1: honour the test hooks (TEST_HOOKS)",
}
TEST_HOOKS = {"NEF_SHARE_GPU", "NEF_DIST_BACKEND", "NEF_DIST_FORCE"}


def get(name, default=None):
    """Value of a PRODUCT switch (`default` when it is unset)."""
    if name not in PRODUCT:
        raise KeyError(f"{name}: not a switch of this package (electrocardio_panorama_amd/_env.py)")
    return os.environ.get(name, default)
