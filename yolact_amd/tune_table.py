"""The shipped tile / algorithm table (`tune/<arch>.json`): its file, its keys and its values, in one place.

    key    [instep|][wino | chain | chain1 | chainx] str(tuple) ['|h2' | '|x3']
           conv    (B, H, W, Cin, Cout, kh, kw, stride, pad, res_mode, nseg, Kpad)   -> direct choice
           dcn     the same 12 ints + 'dcn'                                          -> direct choice
           wino    (B, H, W, C, Cout, act, nseg, (m, ...))    -> [m, Winograd choice, direct ms, Winograd ms, F(2x2) ms, F(4x4) ms]
           chain   (B, H, W[, P])  /  chain1 (B, H, W[, P])  /  chainx (B, H, W)     -> [1 | 0, ms of the plan's launches, ms of the fused one]
                   chain (B, H, W, 64): the ENTRY form of the 64-plane pair (the block's projection shortcut computed inside the pair
                   launch, csrc/chain.hip) -> [1 | 0, ms of the shortcut launch + the pair launch, ms of the entry launch]; the pair's
                   own decision stays under chain (B, H, W), which never spells P for 64 planes
                   wino (B, 4 * tiles, 4, ...): a merged P4..P7 head launch, see level_key
           instep|<wino key>                                                      -> 0: keep the direct kernel (tools/instep_tune.py)
    value  direct choice   = tile id + 256 * split_k (split_k 0 = unsplit)
           Winograd choice = GEMM tile id (+ WINO_PLANES: V written as fp16x2 planes)

Pure Python: torch is imported only where the device's architecture name is looked up; engine.py is never imported.
"""
import ast
import json
import os
import re

from . import _lib as L

TUNE_GEN = 5          # bump whenever tile ids or kernel variants change meaning: older tables are ignored (5: pipelined kernel of csrc/dcn.hip)
TUNE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tune')
_table_cache = {}


# ---- the file ----------------------------------------------------------------------------------------------------------------
def read_table_file(path):
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        return {}
    if not isinstance(doc, dict) or doc.get('gen') != TUNE_GEN or not isinstance(doc.get('abi'), int) or doc['abi'] > L.ABI_VERSION:
        return {}       # (gen = meaning of the tile ids; a table written under an OLDER ABI of the same generation stays valid)
    return dict(doc.get('entries', {}))


def write_table_file(path, entries, device=None, note=None):
    name = None
    if device is not None and device.type == 'cuda':
        import torch
        name = torch.cuda.get_device_name(device)
    doc = {'gen': TUNE_GEN, 'abi': L.ABI_VERSION, 'device': name,
           'note': note or 'tile id per conv shape (B,H,W,Cin,Cout,kh,kw,stride,pad,res_mode,nseg,Kpad); wino(...) -> '
                           '[m, gemm tile, direct ms, winograd ms, F(2x2) ms, F(4x4) ms]',
           'entries': {k: entries[k] for k in sorted(entries)}}
    tmp = path + '.tmp%d' % os.getpid()
    with open(tmp, 'w') as f:
        json.dump(doc, f, indent=0, separators=(',', ':'))
    os.replace(tmp, path)


def load_tune_table(device):
    """Entries of the shipped table for this device's architecture ({} when there is none)."""
    arch = 'gfx950'
    if device.type == 'cuda':
        import torch
        arch = getattr(torch.cuda.get_device_properties(device), 'gcnArchName', 'gfx950').split(':')[0]
    if arch not in _table_cache:
        _table_cache[arch] = read_table_file(os.path.join(TUNE_DIR, arch + '.json'))
    return dict(_table_cache[arch])


def build_meta():
    """yolact_amd/build_meta.json, written by __graft_entry__.build(): {'lint': 'ok' | 'skipped'} (missing file: {})."""
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'build_meta.json')) as f:
            doc = json.load(f)
        return doc if isinstance(doc, dict) else {}
    except (OSError, ValueError):
        return {}


def patch_tile_allowed():
    """csrc/patch.hip issues gfx950's new MFMAs through the plain builtins (no constrained wrapper): what keeps its results right is the
    post-build ISA lint (tools/check_mfma_overlap.py).  A build whose lint could NOT run (build_meta 'lint': 'skipped', only possible
    with YOLACT_AMD_ALLOW_NO_LINT=1) must not select that tile (round-5 advisor); YOLACT_AMD_PATCH=0 is the A/B switch."""
    return os.environ.get('YOLACT_AMD_PATCH', '1') == '1' and build_meta().get('lint', 'ok') != 'skipped'


# ---- keys --------------------------------------------------------------------------------------------------------------------
MODES = ('', 'h2', 'x3')            # exact-fp32 MFMA | fp16x2 | bf16x3 arithmetic of the plan (or, 'x3', of one guarded layer)
KINDS = ('conv', 'dcn', 'wino', 'chain', 'chain1', 'chainx', 'instep')
_PREFIX = {'conv': '', 'dcn': '', 'wino': 'wino', 'chain': 'chain', 'chain1': 'chain1', 'chainx': 'chainx'}
_INSTEP = 'instep|'
_KEY_RE = re.compile(r'(instep\|)?(wino|chain1|chainx|chain|)(\(.*\))(?:\|(h2|x3))?')


def _ints(t, n):
    return len(t) in n and all(type(v) is int for v in t)


def _valid(kind, t):
    if type(t) is not tuple:
        return False
    if kind == 'conv':
        return _ints(t, (12,))
    if kind == 'dcn':
        return len(t) == 13 and _ints(t[:12], (12,)) and t[12] == 'dcn'
    if kind == 'wino':
        return len(t) == 8 and _ints(t[:7], (7,)) and type(t[7]) is tuple and _ints(t[7], (1, 2))
    return _ints(t, (3,) if kind == 'chainx' else (3, 4))


def format(kind, t, mode=''):
    """The table key of (kind, tuple, mode): what parse() takes apart.  'instep' wraps the tuple of a wino key."""
    t = tuple(t)
    inner = 'wino' if kind == 'instep' else kind
    if inner not in _PREFIX or mode not in MODES or not _valid(inner, t):
        raise ValueError('no tune-table key: %r' % ((kind, t, mode),))
    return (_INSTEP if kind == 'instep' else '') + _PREFIX[inner] + str(t) + ('|' + mode if mode else '')


def parse(key):
    """(kind, tuple, mode) of a table key; ValueError on anything format() does not produce."""
    m = _KEY_RE.fullmatch(key) if isinstance(key, str) else None
    try:
        instep, head, t, mode = m.group(1), m.group(2), ast.literal_eval(m.group(3)), m.group(4) or ''
        kind = head or ('dcn' if len(t) == 13 else 'conv')
        if instep:
            kind = {'wino': 'instep'}[kind]
        if format(kind, t, mode) == key:        # (also rejects what str(tuple) would have spelt differently)
            return kind, t, mode
    except (AttributeError, KeyError, TypeError, ValueError, SyntaxError, MemoryError, RecursionError):
        pass
    raise ValueError('no tune-table key: %r' % (key,))


def conv_key(shape, mode='', dcn=False):
    """shape = (B, H, W, Cin, Cout, kh, kw, stride, pad, res_mode, nseg, Kpad) of a direct convolution / of a DCN layer's convolution."""
    return format('dcn', tuple(shape) + ('dcn',), mode) if dcn else format('conv', shape, mode)


def desc_key(d, mode='', dcn=False):
    """conv_key of a ymi_conv_desc."""
    return conv_key((d.B, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad, d.res_mode, d.nseg, d.Kpad), mode, dcn)


def wino_key(B, H, W, C, Cout, act, nseg, ms, mode=''):
    return format('wino', (B, H, W, C, Cout, act, nseg, tuple(ms)), mode)


def level_key(B, tiles, C, Cout, act, nseg, mode=''):
    """The key of a merged P4..P7 head launch (ymi_wino_desc.nlev: several feature maps, one Winograd layer).  No kind of its own:
    a wino key of a VIRTUAL shape no real layer has, (H, W) = (4 * F(4x4) tiles per image over all levels, 4), m = (4,).  Its value
    reads [4 | 0, Winograd choice of the merged GEMM, summed ms of the per-level launches it replaces (where a real layer has its
    direct ms), ms of the merged launch, 0, the same]; the merged form is installed where both entries of a plan (up-feature and
    .out) hold a choice and their merged times sum to less than 0.97 of the per-level sums.  A single map of the virtual shape has
    the merged launch's T = B * tiles GEMM rows, so whatever launches the key as an ordinary layer (the fp64 pin of every shipped
    Winograd entry) runs the merged launch's GEMM shape on its tile."""
    return wino_key(B, 4 * int(tiles), 4, C, Cout, act, nseg, (4,), mode)


def chain_key(kind, B, H, W, P=None, mode=''):
    """kind 'chain' (conv3 + the next conv1) | 'chain1' (conv3 alone); P only for the wider stages of csrc/chain2.hip (P > 64) and,
    as ('chain', ..., 64), for the entry form of the 64-plane pair (the projection shortcut computed in the pair launch)."""
    if kind not in ('chain', 'chain1'):
        raise ValueError(kind)
    return format(kind, (B, H, W) + ((P,) if P is not None else ()), mode)


def chainx_key(B, H, W, mode=''):
    return format('chainx', (B, H, W), mode)


def instep_key(wino):
    """'instep|' + a wino key."""
    kind, t, mode = parse(wino)
    if kind != 'wino':
        raise ValueError('no wino key: %r' % (wino,))
    return format('instep', t, mode)


# ---- values ------------------------------------------------------------------------------------------------------------------
def direct_choice(tile, split_k=0):
    """tile id + 256 * split_k; a split of 0 or 1 is the unsplit launch (stored as 0)."""
    return int(tile) + 256 * (int(split_k) if split_k > 1 else 0)


def direct_parts(v):
    """(tile id, split_k) of a direct choice."""
    return int(v) & 255, int(v) >> 8


def wino_choice(tile, planes=0):
    return int(tile) | (L.WINO_PLANES if planes else 0)


def wino_parts(v):
    """(GEMM tile id, v_planes 1 | 0) of a Winograd choice."""
    return int(v) & 255, 1 if int(v) & L.WINO_PLANES else 0


def choice_name(v):
    """'<tile name>[/k<split_k>]' of a direct choice."""
    tile, S = direct_parts(v)
    return L.TILE_NAMES.get(tile, '?%d' % tile) + ('/k%d' % S if S else '')
