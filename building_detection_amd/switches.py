"""The experiment switches the Python package reads: one table, one accessor.

The native library's switches have their own table (csrc/sg_switch.h); DESIGN.md's appendix describes both.  `get(name)` reads
the environment at EVERY call - tests change these variables between models inside one process - and applies the switch's own
truth rule:

  eq1    on only when the value is exactly "1"      (a value of "2" is off)
  ne0    on unless the value is exactly "0"         (a value of "2" is on)
  flag   on when the variable exists, whatever its value
  int    int(value)
  float  float(value)
"""
import os

# name: (kind, default, effect)
SWITCHES = {
    "SG_BN_ADD": ("eq1", "1", "BatchNormalization layers in front of a residual Add ride in the add kernel; off: their own launch"),
    "SG_BN_SUMS": ("eq1", "1", "BatchNormalization backward sums come from the depthwise dgrad's epilogue; off: their own reduction"),
    "SG_BN_DEFER": ("eq1", "1", "BatchNormalization(+ReLU) in front of a SeparableConv2D is applied in the depthwise gather"),
    "SG_BN_PW": ("eq1", "0", "the BatchNormalization backward apply rides in the A path of the pointwise dgrad (bit-identical, a loss in the step)"),
    "SG_BN_CONV": ("ne0", "1", "BatchNormalization layers in front of thin 1x1 / patch-kernel convolutions ride in their loader; 0: own launch"),
    "SG_THIN_GRAD_BN": ("ne0", "1", "a thin 1x1 convolution's input gradient is evaluated inside the BatchNormalization backward in front of it; 0: written out"),
    "SG_SCSE_LOWRANK": ("ne0", "1", "an scSE block's input gradient is written once, by a final kernel that adds the two gates' rank-one terms; 0: three passes"),
    "SG_ACT_PLANES": ("ne0", "1", "activation planes made once per tensor and step, kept for the planes-in filter gradient; 0: split in every launch"),
    "SG_UP2_FUSE": ("ne0", "1", "UpSampling2D(2) -> Conv2D 3x3 as one sub-pixel launch; 0: a pair of launches"),
    "SG_GRAD_ACC": ("eq1", "1", "the gradient of a two-consumer block input is summed in the dgrad epilogue; off: by a separate add"),
    "SG_PREPARED_PLANES": ("ne0", "1", "weight planes prepared once per optimiser step; 0: rebuilt inside every convolution call"),
    "SG_JIT_LANES": ("ne0", "1", "the captured training step keeps filter gradients on a side lane; 0: inline in one linear graph"),
    "SG_JIT_LANE_BLOCKS": ("int", "24", "filter-gradient blocks per segment of the captured step's side lane"),
    "SG_SIDE_WGRAD": ("int", "1", "filter gradients on the side stream: 1 all, 2 the GEMM ones only, 3 the depthwise ones only, 0 none"),
    "SG_SIDE_KEEP_GIB": ("float", "4", "GiB of side-stream operands held before the main stream joins the side stream and drops them"),
    "SG_TRACE_MARK": ("eq1", "0", "bracket the roofline kernel set with marker kernels for a kernel trace (read once, at import)"),
    "SG_CONV_NOTHIN": ("flag", "", "thin 1x1 streaming kernels off (the library reads the same variable)"),
    "SG_COMM_INIT_TIMEOUT": ("float", "180", "seconds sg_comm_init may take per rank before every rank gives up together"),
}

_RULES = {
    "eq1": lambda v: v == "1",
    "ne0": lambda v: v != "0",
    "int": int,
    "float": float,
}


def get(name: str):
    """The switch's value now: bool for eq1 / ne0 / flag, else int or float."""
    kind, default, _ = SWITCHES[name]
    if kind == "flag":
        return name in os.environ
    return _RULES[kind](os.environ.get(name, default))
