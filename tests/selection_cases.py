"""What the host-side algorithm selection of _hip.py decides, as data: a grid of convolution / weight-gradient problems run through a grid of
switch settings, without a GPU.  `dump(hip)` takes an imported _hip module and returns JSON-able records; tests/golden/selection.json holds the
dump of the commit the selection was last changed in ON PURPOSE, and tests/test_selection_cpu.py compares the working tree with it record by record.

Regenerate (only when a selection change is intended):  python tests/selection_cases.py [path/to/another/_hip.py [its revision]] > tests/golden/selection.json

Nothing here launches: the library answers size queries (y2_conv_fwd_workspace_bytes) on the CPU, everything that would touch a GPU is stubbed inside
`dump`, so the same code serves any revision of _hip.py that keeps its public names."""
import contextlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, 'yolo2-pytorch_amd')
for _p in (ROOT, APP, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = 'cuda:0'
FORCE_ALGOS = ('direct', 'winograd', 'fused', 'implicit', 'fused3', 'implicit3', 'split')
# every switch the grids move, at the value a case starts from (table off, nothing pinned, no measurement)
BASE = dict(_DEFAULTS_SEEN=lambda: {DEV: 0}, TUNE_DEFAULTS=False, TUNE_CACHE=None, TUNE_MISSES=list, AUTOTUNE=False, DETERMINISTIC=False, WINOGRAD=True,
            WGRAD_F34=True, IMPLICIT=True, PERSIST=True, SPLIT='', FORCE_ALGO=None, FORCE_GRAD=None, FORCE_WGRAD=None, SCOPE=None, _LAUNCH=None)
# CPU tensors standing in for the filter operands: only their addresses are used
U, US, U6 = torch.zeros(16), torch.zeros(16), torch.zeros(16)
W_DIRECT, SPLIT_PLANE = 512, 16 * 1280 * 1024          # (the library wants the planes of a split operand at least one operand apart)
# switch cases run over every 416x416 problem (the others: over a dozen of them), and the ones whose answer to peek=True is recorded as well
WIDE = ('deterministic', 'implicit.off', 'winograd.off', 'grad.f43', 'grad.direct', 'split.bf16', 'force.direct', 'force.winograd', 'force.fused', 'force.implicit', 'force.split')
PEEKED = ('deterministic', 'grad.f43', 'grad.direct', 'force.fused')


def load(path, name='_hip_other'):
    """Another revision of _hip.py (e.g. `git show REV:yolo2-pytorch_amd/_hip.py` into a scratch file), reading THIS tree's library and table."""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._HERE = APP
    mod.LIB_PATH = os.environ.get('Y2_LIB') or os.path.join(APP, 'csrc', 'libyolo2_hip.so')
    mod.DEFAULTS_PATH = os.path.join(APP, 'tune', 'default_gfx950.json')
    return mod


class _Table(dict):
    """_hip._TUNE that remembers the keys it was asked for: the key of a problem is a local of autotune_conv / wgrad_choice."""

    def __init__(self, *a):
        dict.__init__(self, *a)
        self.asked = []

    def get(self, key, default=None):
        self.asked.append(key)
        return dict.get(self, key, default)


@contextlib.contextmanager
def _set(obj, **kw):
    old = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


def _switches(hip, **kw):
    """The module's switches at BASE, then `kw`; an empty recording table unless one is given.  Restored on exit."""
    new = {k: (v() if callable(v) else v) for k, v in BASE.items()}
    new['_TUNE'] = _Table()
    new.update(kw)
    return _set(hip, **new)


# ---- problems
def _conv(name, B, H, W, cin, cout, k, y=True, y_pool=False, stats=False, bn=False, implicit_ok=True, grad=False, tags=(), **fields):
    return dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, k=k, y=y, y_pool=y_pool, stats=stats, bn=bn, implicit_ok=implicit_ok, grad=grad, tags=set(tags), fields=fields)


def _params(hip, c):
    p = hip.ConvParams()
    p.x, p.w = 256, W_DIRECT
    p.B, p.H, p.W, p.Cin, p.ldx, p.Cout, p.ksize = c['B'], c['H'], c['W'], c['cin'], c['cin'], c['cout'], c['k']
    p.ldy, p.slope = c['cout'], 0.1
    p.y, p.stats = (256 if c['y'] else None), (256 if c['stats'] else None)
    if c['y_pool']:
        p.y_pool, p.ldp = 256, c['cout']
    if c['bn']:
        p.scale = p.shift = 256
    for f, v in c['fields'].items():
        setattr(p, f, v)
    return p


def problems(hip):
    """(convolution problems, weight-gradient problems).  Darknet-19 at batch 64 and 320 / 416 / 608: every block but the first (its own kernels) as the
    training forward (raw output + statistics; with and without the transformed input kept), the inference forward (y / y_pool as the block has them) and
    the data gradient (Cin / Cout exchanged); the other families' forms and the shapes that reach each special rule of the candidate list."""
    from model import train_graph as tg
    from test_host_logic import _darknet19_geometry
    convs, wgrads, seen = [], [], set()

    def add(c, *ident):
        if ident not in seen:
            seen.add(ident)
            convs.append(c)
    for S in (320, 416, 608):
        tags = ('core',) if S == 416 else ()
        names, geo = _darknet19_geometry(tg, hip, 64, S)
        for name, g in list(zip(names, geo))[1:]:
            shape = (g.H, g.cin, g.cout, g.k)
            n = '%d.%dx%d.%d-%d.k%d' % ((S,) + (g.H, g.W) + shape[1:])
            add(_conv(n + '.train', 64, g.H, g.W, g.cin, g.cout, g.k, stats=True, tags=tags), 'train', shape)
            if g.k == 3:
                add(_conv(n + '.train.keepv', 64, g.H, g.W, g.cin, g.cout, g.k, stats=True, implicit_ok=False, tags=tags), 'keepv', shape)
            y, y_pool = (not g.pooled) or g.full is not None, bool(g.pooled)
            add(_conv(n + '.infer', 64, g.H, g.W, g.cin, g.cout, g.k, y=y, y_pool=y_pool, bn=True), 'infer', shape, y, y_pool)
            if g.k == 3 and g.cout % 4 == 0:
                add(_conv(n + '.dgrad', 64, g.H, g.W, g.cout, g.cin, 3, grad=True, tags=tags), 'dgrad', shape)
            if ('wgrad', shape) not in seen:
                seen.add(('wgrad', shape))
                wgrads.append(dict(name=n, B=64, H=g.H, W=g.W, cin=g.cin, cout=(g.cout + 3) // 4 * 4, k=g.k, tags=set(tags)))
    extra = [
        _conv('resnet.s2.residual', 2, 9, 13, 4, 8, 3, bn=True, residual=256, ldr=8, stride=2, pad_plus1=2),
        _conv('resnet.s1.residual', 32, 26, 26, 256, 256, 3, bn=True, residual=256, ldr=256, stride=1, pad_plus1=2),
        _conv('densenet.coff', 2, 8, 8, 12, 6, 3, ldy=40, coff=22, stride=1, pad_plus1=2),
        _conv('densenet.3x3', 32, 26, 26, 128, 32, 3, ldy=512, coff=256, stride=1, pad_plus1=2),
        _conv('1x1.persistent', 64, 26, 26, 512, 256, 1, bn=True),
        _conv('1x1.persistent.pad1', 32, 13, 13, 1024, 128, 1, stride=1, pad_plus1=1),
        _conv('cin16', 64, 52, 52, 16, 64, 3, bn=True),
        _conv('cout32', 8, 52, 52, 64, 32, 3, bn=True),
        _conv('big.tiles89', 64, 52, 52, 128, 256, 3, bn=True),
        _conv('big.1x1', 64, 104, 104, 64, 128, 1, bn=True),
        _conv('reorg.out_mode1', 64, 26, 26, 512, 64, 1, out_mode=1, ldy=1280),
        _conv('transposed', 8, 13, 13, 64, 64, 3, transposed=1, stride=2, pad_plus1=2, out_h=26, out_w=26),
    ]
    for c in extra:
        c['tags'].add('core')
    return convs + extra, wgrads


# ---- one call, one record
def _operands(hip, c, pruned=False):
    """The keyword arguments model.train_graph._conv would pass for this problem under the module's switches as they are now."""
    from model import train_graph as tg
    eligible = bool(c['fields'].get('out_mode', 0) == 0 and hip.wino_eligible(c['cout'], c['cin'], c['k'], c['fields'].get('stride', 0)))
    u = U if (eligible and not pruned) else None
    f43 = (lambda: U6) if (c['grad'] and tg._f43_offered(eligible, c['cin'], c['H'], c['W'])) else None
    return dict(wino_w=u, implicit_ok=c['implicit_ok'], wino_split=US if u is not None else None, split_plane=SPLIT_PLANE, f43=f43, wino_eligible=eligible)


def _operand_name(w):
    return {W_DIRECT: 'direct', U.data_ptr(): 'u', US.data_ptr(): 'split', U6.data_ptr(): 'u6', None: None}.get(w, '?')


def _after(p):
    return [p.algo, p.tile, _operand_name(p.w), p.w_plane]


def _ask(hip, c, pruned=False, **kw):
    """[key looked up (None: the table was not read), choice, params.algo, .tile, which operand .w is, .w_plane] - or 'OperandMissing' in place of the last five."""
    p = _params(hip, c)
    del hip._TUNE.asked[:]
    try:
        got = hip.autotune_conv(p, DEV, **dict(_operands(hip, c, pruned), **kw))
    except hip.OperandMissing:
        return [_one(hip._TUNE.asked), 'OperandMissing']
    return [_one(hip._TUNE.asked), None if got is None else list(got)] + _after(p)


def _one(keys):
    assert len(keys) <= 1, keys
    return list(keys[0]) if keys else None


class _Events(object):
    """torch.cuda.Event whose elapsed times are scripted."""

    def __init__(self, times):
        self.times = iter(times)

    def __call__(self, enable_timing=False):
        return self

    def record(self):
        pass

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return next(self.times)


class _Lib(object):
    """Stands in for _hip.lib(): every entry point returns `rc` and is written down."""

    def __init__(self, rc=0, on_call=None):
        self.rc, self.names, self.on_call = rc, [], on_call

    def __getattr__(self, name):
        def fn(*a):
            if name == 'y2_wino_wgrad_ex':                          # with the form it was asked for
                self.names.append('%s:%d' % (name, a[13]))
            elif name == 'y2_wino_wgrad_workspace_bytes_ex':
                self.names.append('scratch_ex:%d' % a[5])
            else:
                self.names.append(name)
            if self.on_call is not None:
                self.on_call(name)
            return self.rc
        return fn


def _candidates(hip, c):
    """The measuring branch with nothing launched: [key stored, (algo, tile) in the order they would be timed, (algo, operand, w_plane, stats set) as launched, choice, params after]."""
    tried, reads, stored = [], [], []
    p = _params(hip, c)

    def no_workspace(params, dev):
        tried.append([params.algo, params.tile])
        how = [params.algo, _operand_name(params.w), params.w_plane, bool(params.stats)]
        if how not in reads:
            reads.append(how)
        return -1
    with _set(hip, conv_workspace=no_workspace, stream=lambda: None, tune_store=lambda key, value: stored.append([list(key), value])), \
            _set(torch.cuda, is_current_stream_capturing=lambda: False):
        got = hip.autotune_conv(p, DEV, **_operands(hip, c))
    return [stored, tried, reads, list(got)] + _after(p) + [bool(p.stats)]


def _timed(hip, c, times):
    """The measuring branch on scripted times: [choice, stored, y2_conv_fwd launches, was params.stats ever set while launching]."""
    stored, seen_stats = [], set()
    p = _params(hip, c)
    fake = _Lib(on_call=lambda name: seen_stats.add(bool(p.stats)))
    with _set(hip, conv_workspace=lambda params, dev: 0, stream=lambda: None, lib=lambda: fake, tune_store=lambda key, value: stored.append([list(key), value])), \
            _set(torch.cuda, is_current_stream_capturing=lambda: False, Event=_Events(times)):
        got = hip.autotune_conv(p, DEV, **_operands(hip, c))
    return [list(got), stored, fake.names.count('y2_conv_fwd'), sorted(seen_stats), bool(p.stats)]


def _wgrad_run(hip, w, times=None, capturing=False, has_v=False, **kw):
    """conv_wgrad on stand-ins: [entry points called (y2_wino_wgrad_ex and its scratch query with their mode; the other size queries left out), choices stored]."""
    stored = []
    fake = _Lib(rc=4096)
    x, dz = torch.zeros(4), torch.zeros(4)
    out = torch.zeros(w['cout'] * w['cin'] * w['k'] * w['k'])
    with _set(hip, lib=lambda: fake, check=lambda rc, what: None, stream=lambda: None, tune_store=lambda key, value: stored.append([list(key), value])), \
            _set(torch.cuda, is_current_stream_capturing=lambda: capturing, Event=_Events(times or [])):
        hip.conv_wgrad(x, dz, w['B'], w['H'], w['W'], w['cin'], w['cin'], w['cout'], w['cout'], w['k'], v=torch.zeros(4) if has_v else None, out=out, **kw)
    return [_runs([n for n in fake.names if 'workspace' not in n]), stored]


def _wgrad_ask(hip, w, has_v):
    del hip._TUNE.asked[:]
    got = hip.wgrad_choice(w['B'], w['H'], w['W'], w['cin'], w['cin'], w['cout'], w['cout'], w['k'], has_v, DEV)
    return [_one(hip._TUNE.asked), got]


def dump(hip):
    """{'keys': [...], 'problems': [...], 'cases': {case: [[problem, key, what was decided ...], ...]}}: a record names its problem and the table key it
    asked for (or stored under) by their index in the two lists - most cases ask the same few hundred keys."""
    convs, wgrads = problems(hip)
    core = [c for c in convs if 'core' in c['tags']]
    core_w = [w for w in wgrads if 'core' in w['tags']]
    few = [c for c in core if c['name'].split('.')[-1] in ('keepv', 'dgrad', 'persistent')][:12]
    keys, names, index, cases = [], [c['name'] for c in convs + wgrads], {}, {}

    def intern(key):
        if key is None:
            return None
        t = json.dumps(key)
        if t not in index:
            index[t] = len(keys)
            keys.append(key)
        return index[t]

    def rec(case, c, r):
        cases.setdefault(case, []).append([names.index(c['name']), intern(r[0])] + r[1:])
    # the committed table, asked without applying; then applied where it answers, with and without the Winograd operand at hand
    with _switches(hip, _DEFAULTS_SEEN={}, TUNE_DEFAULTS=True, AUTOTUNE=True):
        for c in convs:
            r = _ask(hip, c, peek=True)
            rec('table.peek', c, r)
            if r[1] is not None and 'core' in c['tags']:
                rec('table.apply', c, _ask(hip, c))
                rec('table.apply.pruned', c, _ask(hip, c, pruned=True))
        for w in wgrads:
            for has_v in (True, False):
                rec('wgrad.table.v%d' % has_v, w, _wgrad_ask(hip, w, has_v))
    # table off, no measurement: the static preferences through the library's own acceptance test
    with _switches(hip):
        for c in convs:
            rec('static', c, _ask(hip, c))
        for c in core:
            rec('static.pruned', c, _ask(hip, c, pruned=True))
            rec('choice.given', c, _ask(hip, c, choice=(0, 3)))
        for w in wgrads:
            rec('wgrad.static', w, _wgrad_ask(hip, w, True))
    for case, kw in [('deterministic', dict(DETERMINISTIC=True, AUTOTUNE=True)), ('implicit.off', dict(IMPLICIT=False)), ('winograd.off', dict(WINOGRAD=False)),
                     ('grad.f43', dict(FORCE_GRAD='f43')), ('grad.direct', dict(FORCE_GRAD='direct')),
                     ('split.bf16', dict(SPLIT='bf16')), ('split.f16', dict(SPLIT='f16')), ('split.true', dict(SPLIT=True))] + \
                    [('force.' + a, dict(FORCE_ALGO=a, AUTOTUNE=True, SPLIT='bf16' if a == 'split' else '')) for a in FORCE_ALGOS] + \
                    [('force.split.f16', dict(FORCE_ALGO='split', SPLIT='f16')), ('force.split.off', dict(FORCE_ALGO='split', SPLIT=''))]:
        with _switches(hip, **kw):
            for c in (core if case in WIDE else few):
                if case in PEEKED:
                    rec(case + '.peek', c, _ask(hip, c, peek=True))
                rec(case, c, _ask(hip, c))
    # a table entry that names a persistent tile, with and without Y2_CONV_PERSIST; a scalar entry (tile only) of an old table; deterministic mode over an entry
    for c in core:
        if c['k'] != 1:
            continue
        with _switches(hip, AUTOTUNE=True):
            key = _candidates(hip, c)[0][0][0]
        for case, kw, entry in [('persist.on', {}, [0, 13]), ('persist.off', dict(PERSIST=False), [0, 13]), ('persist.off.plain', dict(PERSIST=False), [0, 3]),
                                ('entry.scalar', {}, 2), ('entry.deterministic', dict(DETERMINISTIC=True), [0, 3])]:
            with _switches(hip, _TUNE=_Table({tuple(key): entry}), **kw):
                rec(case + '.peek', c, _ask(hip, c, peek=True))
                rec(case, c, _ask(hip, c))
    # what a measurement would time, in order
    for case, kw in [('candidates', {}), ('candidates.split.bf16', dict(SPLIT='bf16')), ('candidates.split.f16', dict(SPLIT='f16')), ('candidates.persist.off', dict(PERSIST=False)),
                     ('candidates.implicit.off', dict(IMPLICIT=False)), ('candidates.winograd.off', dict(WINOGRAD=False))]:
        with _switches(hip, AUTOTUNE=True, **kw):
            for c in (core if case == 'candidates' else few):
                r = _candidates(hip, c)
                assert len(r[0]) == 1 and r[0][0][1] == [0, 0], r[0]          # nothing was accepted: the direct kernel, stored under the problem's key
                rec(case, c, [r[0][0][0]] + r[1:])
    # the timing protocol on scripted times: 1 launch + 3 x 3 per candidate, best batch counts, a tie goes to the earlier candidate
    with _switches(hip, AUTOTUNE=True):
        timed = [c for c in core if c['name'] in ('416.13x13.512-1024.k3.dgrad', '416.52x52.128-256.k3.train', '1x1.persistent', 'cin16')]
        assert len(timed) == 4
        for c in timed:
            n = 3 * len(_candidates(hip, c)[1])
            for case, times in [('timed.ties', [3 + (i * 7) % 5 for i in range(n)]), ('timed.flat', [1.0] * n), ('timed.last', [float(n - i) for i in range(n)])]:
                r = _timed(hip, c, times)
                rec(case, c, [r[1][0][0], r[0], r[1][0][1]] + r[2:])
    # weight gradient: the pins, the modes, the rule of a captured step, the measurement
    for case, kw in [('wgrad.force.' + f, dict(FORCE_WGRAD=f, AUTOTUNE=True)) for f in ('direct', 'wino', 'f34')] + \
                    [('wgrad.deterministic', dict(DETERMINISTIC=True, AUTOTUNE=True)), ('wgrad.force.f34.deterministic', dict(FORCE_WGRAD='f34', DETERMINISTIC=True)),
                     ('wgrad.f34.off', dict(WGRAD_F34=False)), ('wgrad.winograd.off', dict(WINOGRAD=False)), ('wgrad.unknown', dict(AUTOTUNE=True))]:
        with _switches(hip, **kw):
            for w in core_w:
                rec(case, w, _wgrad_ask(hip, w, True))
    with _switches(hip, AUTOTUNE=True):
        for w in core_w:
            if w['k'] != 3 or w['cin'] < 32:
                continue
            rec('wgrad.capturing', w, [None] + _wgrad_run(hip, w, capturing=True))
            for has_v in (False, True):
                # direct 1.0, 2x2 tiles 0.9, 4x4 tiles 1.2 (best of two batches each): the forward-cost correction of the large maps decides
                r = _wgrad_run(hip, w, times=[1.0, 1.1, 0.95, 0.9, 1.2, 1.3], has_v=has_v)
                rec('wgrad.timed.v%d' % has_v, w, [r[1][0][0], r[0], r[1][0][1]])
            with _set(hip, WGRAD_F34=False):
                r = _wgrad_run(hip, w, times=[1.0, 1.1, 1.2, 1.05])
                rec('wgrad.timed.f34.off', w, [r[1][0][0], r[0], r[1][0][1]])
            for choice in (0, 1, 2):
                rec('wgrad.given.%d' % choice, w, [None] + _wgrad_run(hip, w, choice=choice))
                rec('wgrad.given.%d.native' % choice, w, [None] + _wgrad_run(hip, w, choice=choice, native=torch.zeros(w['cout'], w['cin'], 3, 3), zeroed=True))
            rec('wgrad.given.pre', w, [None] + _wgrad_run(hip, w, choice=2, dz_pre=True))
            rec('wgrad.given.pre.native', w, [None] + _wgrad_run(hip, w, choice=2, dz_pre=True, native=torch.zeros(w['cout'], w['cin'], 3, 3)))
    return json.loads(json.dumps({'keys': keys, 'problems': names, 'cases': cases}))


def differences(want, got):
    """Readable mismatches between two dumps, record by record (problems and keys resolved): [] when they agree."""
    def resolve(d):
        return {case: [[d['problems'][r[0]], None if r[1] is None else d['keys'][r[1]]] + r[2:] for r in rs] for case, rs in d['cases'].items()}
    a, b = resolve(want), resolve(got)
    out = ['case %s: expected, not produced' % c for c in a if c not in b] + ['case %s: produced, not expected' % c for c in b if c not in a]
    for case in a:
        ra, rb = a[case], b.get(case, a[case])
        if len(ra) != len(rb):
            out.append('case %s: %d records expected, %d produced' % (case, len(ra), len(rb)))
        out += ['%s %s: expected %r, got %r' % (case, x[0], x[1:], y[1:]) for x, y in zip(ra, rb) if x != y]
    return out


def _runs(names):
    """['a', 'a', 'b'] -> ['a*2', 'b']."""
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return [n if k == 1 else '%s*%d' % (n, k) for n, k in out]


if __name__ == '__main__':
    if len(sys.argv) > 1:
        module = load(sys.argv[1])
    else:
        import _hip as module
    d = dump(module)
    print('{"source": %s,' % json.dumps(sys.argv[2] if len(sys.argv) > 2 else 'working tree'))
    print('"problems": %s,' % json.dumps(d['problems']))
    print('"keys": [\n%s\n],' % ',\n'.join(json.dumps(k, separators=(',', ':')) for k in d['keys']))
    print('"cases": {\n%s\n}}' % ',\n'.join('%s: [\n%s\n]' % (json.dumps(c), ',\n'.join(json.dumps(r, separators=(',', ':')) for r in rs)) for c, rs in d['cases'].items()))
