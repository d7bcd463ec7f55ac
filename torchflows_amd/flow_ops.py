"""What the flow-program compiler, the packers and the route share about the kernels: the op codes of include/tfk.h
(``tfk_op_kind``), the operand-format flags of an op's fifth field, the table of lean kinds, the constants of the lean
pre-scaling and the LDS budgets of a launch."""
from __future__ import annotations

from collections import namedtuple

# enum tfk_op_kind (include/tfk.h); tests/test_host_program_routes.py checks the two against each other
OP_EW_MULADD, OP_EW_SUBDIV, OP_AFFINE_FWD, OP_AFFINE_INV, OP_SHIFT_FWD, OP_SHIFT_INV, \
    OP_RQS_FWD, OP_RQS_INV, OP_MADE_FWD, OP_MADE_INV, OP_MADE_RQS, OP_PLANE_SWAP, \
    OP_AFFINE_FWD_LEAN, OP_AFFINE_INV_LEAN, OP_SHIFT_FWD_LEAN, OP_SHIFT_INV_LEAN, OP_EW_FMA, \
    OP_RQS_FWD_LEAN, OP_RQS_INV_LEAN, OP_EWC_MULADD, OP_EWC_SUBDIV, OP_MADE_FWD_LEAN, OP_MADE_INV_LEAN, \
    OP_LRS_FWD_LEAN, OP_LRS_INV_LEAN, OP_MADE_RQS_FWD_LEAN, OP_MADE_RQS_INV_LEAN, OP_MADE_LRS_FWD_LEAN, \
    OP_MADE_LRS_INV_LEAN = range(29)
FORWARD, INVERSE = 0, 1

# fifth field of an op record: the bin count of a spline op in the low byte, the operand format of a lean op's GEMM 2 above it
N_BINS = 8                # the fused spline ops are built for the default 8 bins
FMT_BF16X3 = 256          # three bf16 pieces per weight (csrc/tfk_flow_chain.h: couple_lean3, tfk_flow_rqs_chain.h)
FMT_F16X2 = 512           # split f16, hi + lo (csrc/tfk_flow_chain.h: couple_lean_h)

MAX_CONTEXT = 16      # context elements a flow program takes (4 k-steps of 4, csrc/tfk_flow_mfma.h: kCtxSteps)
LOG2E = 1.4426950408889634
AFF_C0 = -1.000000082790371e-10       # float32(log(1 - 1e-10)), affine.py:19-23
RQS_PAD = 24          # 23 spline parameters per element, padded to 6 float4
MAX_HIDDEN_RQS = 32

# parameters staged in LDS per launch; 40 KB keeps 4 workgroups (16 waves) per CU and holds
# the whole RealNVP(64, n_layers=8) program (35.8 KB)
MAX_PARAM_BYTES = 40 * 1024
# the matrix-core layout stores MFMA A-operands per lane (zero-padded to 16 hidden units):
# RealNVP(64, n_layers=8) is 49 KB; its kernel runs 512-thread workgroups, 2 per CU (register-bound)
MAX_PARAM_BYTES_MFMA = 52 * 1024
# wider rows hold more registers per lane, so fewer workgroups fit a CU whatever the LDS use:
# D = 128 (120 VGPRs) runs 2 x 512 threads per CU, D = 256 (179 VGPRs) one -- their launches may
# stage more of the program (each extra launch re-reads and re-writes all the rows)
MFMA_BUDGET_WIDE = {128: 76 * 1024, 256: 150 * 1024}
LEAN_BUDGET_64 = 76 * 1024        # lean affine / shift chains at D = 64 (two 512-thread workgroups per CU either way)
LDS_LIMIT = 150 * 1024            # what one workgroup can stage at all: no op, and no launch, holds more
MAX_OPS = 96
MAX_OPS_LEAN = 60


# One kind of layer the lean programs (csrc/tfk_flow_chain.h, tfk_flow_rqs_chain.h) run, by lean kind ``lk``:
#   op          op code
#   family      affine, shift, rqs, lrs (couplings) | made, made_rqs, made_lrs (MADE layers, parallel map)
#   inverse     the dividing form of an affine map / the inverse of a shift or a spline
#   streamed    operands are read from global memory, chunk by chunk, not staged in LDS
#   spline
#   params      conditioner outputs per element
#   max_hidden  widest hidden layer the kind exists for
LeanKind = namedtuple("LeanKind", "op family inverse streamed spline params max_hidden")


LEAN_KINDS = {
    0: LeanKind(OP_AFFINE_FWD_LEAN, "affine", False, False, False, 2, 16),
    1: LeanKind(OP_AFFINE_INV_LEAN, "affine", True, False, False, 2, 16),
    2: LeanKind(OP_SHIFT_FWD_LEAN, "shift", False, False, False, 1, 16),
    3: LeanKind(OP_SHIFT_INV_LEAN, "shift", True, False, False, 1, 16),
    4: LeanKind(OP_RQS_FWD_LEAN, "rqs", False, True, True, 23, 31),
    5: LeanKind(OP_RQS_INV_LEAN, "rqs", True, True, True, 23, 31),
    6: LeanKind(OP_MADE_FWD_LEAN, "made", False, False, False, 2, 16),
    7: LeanKind(OP_MADE_INV_LEAN, "made", True, False, False, 2, 16),
    8: LeanKind(OP_LRS_FWD_LEAN, "lrs", False, True, True, 32, 31),
    9: LeanKind(OP_LRS_INV_LEAN, "lrs", True, True, True, 32, 31),
    10: LeanKind(OP_MADE_RQS_FWD_LEAN, "made_rqs", False, True, True, 23, 15),
    # (11 and OP_MADE_*_INV_LEAN: the inverse of a MADE spline layer is its sequential map, never a program)
    12: LeanKind(OP_MADE_LRS_FWD_LEAN, "made_lrs", False, True, True, 32, 15),
}
LEAN_BY_OP = {k.op: k for k in LEAN_KINDS.values()}
COUPLING_FAMILIES = ("affine", "shift", "rqs", "lrs")


def lean_kind(family: str, inverse: bool = False) -> int:
    """``lk`` of a family and direction."""
    return next(lk for lk, k in LEAN_KINDS.items() if k.family == family and k.inverse == inverse)
