"""Case table of the depthwise-convolution tests (tests/test_gpu_dwconv.py runs it on the GPU, tests/test_dw_cases.py proves on the CPU that
every case reaches what it claims), and the Python mirror of the host code of csrc/dwconv.hip that shapes a launch:

    dw_grid          CV, Cg, TC, TP, gy, gx, whether gx was capped, pixels per thread, a last channel block with idle lanes
    dw_vec_ok        the 16-B / scalar decision, as a function of C, the two pixel strides and the two bases' offsets from a 16-B boundary
    dw_shape_ok      the refusals, Ho / Wo, the pixel counts
    y2_dwconv_wgrad_workspace_bytes

Plain integer arithmetic in the host code's order.  A case names, per entry point, the claims it is there for; a claim the mirror does not
confirm fails the CPU test, so a change of the grid heuristics that silently moves a case to another path is noticed there.

Left out on purpose: a CAPPED grid of the min_pix = 8 kernel (dwconv_wgrad_kernel).  Its threads already take 2 to 8 steps at the shapes below
(the cap only lengthens the same loop), and reaching it needs operands of 8 * 2048 * 256 * CV / gy elements: 4 M (CV = 1) to 17 M (CV = 4)."""
import collections

DW_THREADS = 256                # csrc/dwconv.hip DW_THREADS
NUM_CU = 256                    # csrc/common.h Y2_NUM_CU
DW_MAX_BLOCKS = NUM_CU * 8      # csrc/dwconv.hip DW_MAX_BLOCKS
DW_WGRAD_MIN_PIX = 8            # csrc/dwconv.hip DW_WGRAD_MIN_PIX
STATS_REPL = 32                 # include/yolo2_hip.h Y2_STATS_REPL
PIX_LIMIT = 0x7fffffff          # dw_shape_ok: pixel indices are 32-bit

Grid = collections.namedtuple('Grid', 'CV Cg TC TP gy gx capped steps ragged')
Shape = collections.namedtuple('Shape', 'Pin Pout Ho Wo')


def dw_grid(P, C, CV, min_pix):
    """dw_grid of csrc/dwconv.hip (pe_grid of csrc/dense.hip is the same function).  steps: pixels the busiest thread visits; ragged: the last
    channel block has idle lanes."""
    Cg = C // CV
    TC = 1
    while TC < Cg and TC < 64:
        TC *= 2
    TP = DW_THREADS // TC
    gy = (Cg + TC - 1) // TC
    gx = (P + TP * min_pix - 1) // (TP * min_pix)
    cap = DW_MAX_BLOCKS // gy
    if cap < 1:
        cap = 1
    capped = gx > cap
    if capped:
        gx = cap
    if gx < 1:
        gx = 1
    steps = (P + gx * TP - 1) // (gx * TP)
    return Grid(CV, Cg, TC, TP, gy, gx, capped, steps, Cg % TC != 0)


def dw_vec_ok(C, lda, ldb, offa, offb):
    """offa / offb: the bases' distance in floats from a 16-byte boundary."""
    return not (C & 3) and not (lda & 3) and not (ldb & 3) and not (offa & 3) and not (offb & 3)


def dw_shape_ok(B, H, W, C, stride):
    """None where every entry point answers Y2_EINVAL (the workspace query 0)."""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or stride not in (1, 2):
        return None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Pin, Pout = B * H * W, B * Ho * Wo
    return Shape(Pin, Pout, Ho, Wo) if Pin < PIX_LIMIT else None


def wgrad_workspace_bytes(B, H, W, C, stride):
    s = dw_shape_ok(B, H, W, C, stride)
    if s is None:
        return 0
    gx = 0
    for CV in (1, 4):
        if CV == 4 and C & 3:
            continue
        gx = max(gx, dw_grid(s.Pout, C, CV, DW_WGRAD_MIN_PIX).gx)
    return gx * C * 9 * 4


def wgrad_need_bytes(B, H, W, C, stride, CV):
    return dw_grid(dw_shape_ok(B, H, W, C, stride).Pout, C, CV, DW_WGRAD_MIN_PIX).gx * C * 9 * 4


# entry point: (its two activation operands in dw_vec_ok's order, which pixel count it walks, min_pix)
ENTRIES = collections.OrderedDict([('fwd', (('x', 'y'), 'Pout', 1)), ('dgrad', (('dz', 'dx'), 'Pin', 1)), ('wgrad', (('x', 'dz'), 'Pout', DW_WGRAD_MIN_PIX))])
OPERANDS = ('x', 'y', 'dz', 'dx')        # x, dx: [B,H,W]; y, dz: [B,Ho,Wo]

# shape (B, C, H, W, stride); pad: ld - C per operand (x, y, dz, dx); off: base offset in floats from a 16-B boundary per operand; claims per entry
Case = collections.namedtuple('Case', 'shape pad off claims')


def _case(shape, pad, off, fwd, dgrad, wgrad):
    return Case(shape, dict(zip(OPERANDS, pad)), dict(zip(OPERANDS, off)), {'fwd': fwd.split(), 'dgrad': dgrad.split(), 'wgrad': wgrad.split()})


A = (0, 0, 0, 0)
CASES = collections.OrderedDict((n, _case(*v)) for n, v in [
    # ---- the grid cap: a thread walks two or more pixels, the statistics reduction follows such a walk
    ('v4-gy4-capped', ((1, 1024, 47, 47, 1), (4, 8, 12, 0), A,
                       'cv4 gy>1 capped walk>=2 TC64 stats-copies>32 stride1', 'cv4 gy>1 capped walk>=2 TC64', 'cv4 gy>1 walk>=2')),
    ('v4-gy1-capped', ((1, 256, 91, 91, 1), (0, 4, 8, 12), A,
                       'cv4 gy1 capped walk>=2 TC64 stats-copies>32', 'cv4 gy1 capped walk>=2 TC64', 'cv4 gy1 walk>=2 TC64')),
    ('v4-gy2-ragged-capped', ((1, 288, 65, 65, 1), (0, 4, 8, 12), A,
                              'cv4 gy>1 ragged-channel-block capped walk>=2 TC64 stats-copies>32',
                              'cv4 gy>1 ragged-channel-block capped walk>=2', 'cv4 gy>1 ragged-channel-block walk>=2')),
    ('v1-gy2-ragged-capped', ((1, 70, 65, 65, 1), (0, 1, 2, 5), A,
                              'cv1 cv1-by-C gy>1 ragged-channel-block capped walk>=2 TC64 stats-copies>32 stride1',
                              'cv1 gy>1 ragged-channel-block capped walk>=2', 'cv1 gy>1 ragged-channel-block walk>=2')),
    ('v1-gy2-ragged-capped-s2', ((1, 70, 129, 131, 2), (2, 0, 3, 1), A,
                                 'cv1 gy>1 ragged-channel-block capped walk>=2 stride2 odd-map stats-copies>32',
                                 'cv1 gy>1 ragged-channel-block capped walk>=2 stride2 odd-map', 'cv1 gy>1 ragged-channel-block walk>=2 stride2 odd-map')),
    ('v1-gy1-capped', ((1, 6, 257, 256, 1), (0, 1, 2, 3), A,
                       'cv1 cv1-by-C gy1 capped walk>=2 TC8 stats-copies>32', 'cv1 gy1 capped walk>=2 TC8', 'cv1 gy1 walk>=2 TC8')),
    # ---- several channel blocks, the last with idle lanes, one pixel per thread
    ('v4-gy2-ragged', ((2, 288, 9, 7, 1), (4, 0, 8, 12), A,
                       'cv4 gy>1 ragged-channel-block walk1 TC64 stride1', 'cv4 gy>1 ragged-channel-block walk1', 'cv4 gy>1 ragged-channel-block')),
    ('v4-gy2-ragged-s2', ((2, 288, 9, 7, 2), (0, 8, 4, 12), A,
                          'cv4 gy>1 ragged-channel-block walk1 stride2 odd-map', 'cv4 gy>1 ragged-channel-block walk1 stride2 odd-map',
                          'cv4 gy>1 ragged-channel-block stride2 odd-map')),
    ('v1-gy3-ragged', ((2, 130, 9, 7, 1), (0, 3, 1, 2), A,
                       'cv1 cv1-by-C gy>1 ragged-channel-block walk1 TC64', 'cv1 cv1-by-C gy>1 ragged-channel-block walk1', 'cv1 cv1-by-C gy>1 ragged-channel-block')),
    ('v1-gy2-ragged-s2-even', ((2, 70, 8, 6, 2), (1, 0, 0, 3), A,
                               'cv1 gy>1 ragged-channel-block walk1 stride2 even-map', 'cv1 gy>1 ragged-channel-block walk1 stride2 even-map',
                               'cv1 gy>1 ragged-channel-block stride2 even-map')),
    # ---- one channel block
    ('v4-gy1', ((2, 36, 7, 9, 1), (0, 4, 8, 12), A, 'cv4 gy1 walk1 TC16 stride1', 'cv4 gy1 walk1 TC16', 'cv4 gy1 TC16')),
    ('v4-gy1-s2-even', ((1, 36, 8, 6, 2), (4, 0, 12, 8), A, 'cv4 gy1 walk1 stride2 even-map', 'cv4 gy1 walk1 stride2 even-map', 'cv4 gy1 stride2 even-map')),
    ('v4-TC1', ((2, 4, 11, 5, 1), (0, 4, 8, 12), A, 'cv4 gy1 walk1 TC1', 'cv4 gy1 walk1 TC1', 'cv4 gy1 TC1')),
    ('v4-TC2', ((2, 8, 11, 5, 1), (4, 0, 12, 8), A, 'cv4 gy1 walk1 TC2', 'cv4 gy1 walk1 TC2', 'cv4 gy1 TC2')),
    ('v1-gy1', ((2, 6, 5, 7, 1), (2, 6, 10, 14), A, 'cv1 cv1-by-C gy1 walk1 TC8', 'cv1 cv1-by-C gy1 walk1 TC8', 'cv1 cv1-by-C gy1 TC8')),
    ('v1-TC1', ((3, 1, 5, 4, 2), (0, 2, 1, 3), A, 'cv1 gy1 walk1 TC1 stride2', 'cv1 gy1 walk1 TC1', 'cv1 gy1 TC1')),
    ('v4-1x1', ((3, 32, 1, 1, 1), (0, 4, 8, 12), A, 'cv4 gy1 walk1 1x1-map TC8', 'cv4 1x1-map', 'cv4 1x1-map')),
    ('v4-1x1-s2', ((3, 32, 1, 1, 2), (4, 0, 12, 8), A, 'cv4 1x1-map stride2 odd-map', 'cv4 1x1-map stride2', 'cv4 1x1-map stride2')),
    # ---- the scalar path for exactly one reason: one base 4-byte aligned only, or one stride that is not a multiple of 4 (C = 40 could go 16-B)
    ('ptr-x', ((2, 40, 6, 5, 1), (0, 4, 8, 12), (1, 0, 0, 0), 'cv1 cv1-by-ptr:x TC64 gy1', 'cv4', 'cv1 cv1-by-ptr:x')),
    ('ptr-y', ((2, 40, 6, 5, 1), (0, 4, 8, 12), (0, 3, 0, 0), 'cv1 cv1-by-ptr:y', 'cv4', 'cv4')),
    ('ptr-dz', ((2, 40, 6, 5, 2), (0, 4, 8, 12), (0, 0, 2, 0), 'cv4', 'cv1 cv1-by-ptr:dz stride2', 'cv1 cv1-by-ptr:dz stride2')),
    ('ptr-dx', ((2, 40, 6, 5, 1), (0, 4, 8, 12), (0, 0, 0, 1), 'cv4', 'cv1 cv1-by-ptr:dx', 'cv4')),
    ('stride-x', ((2, 40, 6, 5, 1), (1, 4, 8, 12), A, 'cv1 cv1-by-stride cv1-by-stride:x', 'cv4', 'cv1 cv1-by-stride cv1-by-stride:x')),
    ('stride-y', ((2, 40, 6, 5, 2), (0, 2, 8, 12), A, 'cv1 cv1-by-stride cv1-by-stride:y stride2', 'cv4', 'cv4')),
    ('stride-dz', ((2, 40, 6, 5, 1), (0, 4, 3, 12), A, 'cv4', 'cv1 cv1-by-stride cv1-by-stride:dz', 'cv1 cv1-by-stride cv1-by-stride:dz')),
    ('stride-dx', ((2, 40, 6, 5, 1), (0, 4, 8, 5), A, 'cv4', 'cv1 cv1-by-stride cv1-by-stride:dx', 'cv4')),
])

# forward epilogue forms, run on one case per CV (both with several channel blocks)
FORM_CASES = ('v4-gy2-ragged', 'v1-gy3-ragged')
FORMS = ('plain', 'affine-relu', 'affine-slope0.1', 'scale-only', 'shift-only')
MAX_ELEMENTS = 2400000          # the largest operand of the table, in floats


def ld(case, operand):
    return case.shape[1] + case.pad[operand]


def derive(case, entry):
    """Everything the mirror can say about the launch of `entry` for `case`, in the claim vocabulary."""
    B, C, H, W, stride = case.shape
    s = dw_shape_ok(B, H, W, C, stride)
    (a, b), pix, min_pix = ENTRIES[entry]
    vec = dw_vec_ok(C, ld(case, a), ld(case, b), case.off[a], case.off[b])
    g = dw_grid(getattr(s, pix), C, 4 if vec else 1, min_pix)
    out = {'cv%d' % g.CV, 'TC%d' % g.TC, 'stride%d' % stride, 'gy1' if g.gy == 1 else 'gy>1', 'walk1' if g.steps == 1 else 'walk>=2'}
    if not vec:
        if C & 3:
            out.add('cv1-by-C')
        for o in (a, b):
            if ld(case, o) & 3:
                out |= {'cv1-by-stride', 'cv1-by-stride:' + o}
            if case.off[o] & 3:
                out.add('cv1-by-ptr:' + o)
    if g.capped:
        out.add('capped')
    if g.gy > 1 and g.ragged:
        out.add('ragged-channel-block')
    if entry == 'fwd' and g.gx > STATS_REPL:
        out.add('stats-copies>32')
    if stride == 2:
        out.add('odd-map' if (H & 1) and (W & 1) else ('even-map' if not (H & 1) and not (W & 1) else 'mixed-map'))
    if H == 1 and W == 1:
        out.add('1x1-map')
    return out, g


def scalar_reasons(case, entry):
    """Why the launch is scalar: 'cv1-by-C', 'cv1-by-stride:<operand>', 'cv1-by-ptr:<operand>' - one element where there is exactly one reason."""
    return {c for c in derive(case, entry)[0] if c.startswith('cv1-by-') and c != 'cv1-by-stride'}
