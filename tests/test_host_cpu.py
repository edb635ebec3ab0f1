"""CPU tests (no GPU): the C-ABI library loads and exports every symbol the header declares, host-side
logic of the training loop, the model surface (state_dict keys / attributes of the reference), and
the world_size-2 data-parallel path over gloo."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_loads_and_exports_header_symbols():
    from deepards_amd import _lib
    _lib.build()
    lib = _lib.lib()
    syms = _lib.header_symbols()
    assert len(syms) >= 20
    assert set(syms) == set(_lib.SIGNATURES)
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.da_version() >= 100
    # pure host helpers of the ABI (no GPU needed)
    assert lib.da_conv_wgrad_workspace(1280, 56, 64, 64, 3) % (3 * 64 * 64 * 4) == 0
    assert lib.da_stem_wgrad_workspace(1280, 64) == 512 * 64 * 7 * 4


def test_every_quoted_include_is_a_rebuild_dependency():
    """_lib.build() rebuilds when a file of _lib.HEADERS is newer than the library: every `#include "..."` of csrc/ must name
    one of them, or an edit to that header leaves a stale library behind."""
    import re
    from deepards_amd import _lib
    assert _lib.HEADERS == sorted(_lib.HEADERS) and {'common.h', 'se_tail.h', 'layer_shared.h'} <= set(_lib.HEADERS)
    files = sorted(f for f in os.listdir(_lib.CSRC) if f.endswith(('.hip', '.h')))
    assert set(_lib.SOURCES) | set(_lib.HEADERS) == set(files)
    for f in files:
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(_lib.CSRC, f)).read(), flags=re.M):
            assert inc in _lib.HEADERS, '%s includes "%s"' % (f, inc)


def test_abi_structs_agree_between_header_library_and_binding(tmp_path):
    """The descriptor structs exist three times: in the public header, in the library's sources and as ctypes mirrors.
    sizeof of each must agree: header compiled by gcc, da_abi_sizes() of the built library, ctypes.sizeof."""
    import ctypes
    import subprocess
    from deepards_amd import _lib
    src = tmp_path / 'abi.c'
    src.write_text('#include <stdio.h>\n#include "deepards_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(da_wgrad_job), sizeof(da_conv_job), sizeof(da_wgrad_reduce_desc), sizeof(da_repack_desc), '
                   'sizeof(da_bn_running_desc), sizeof(da_bn_pgrad_desc)); return 0; }\n')
    exe = tmp_path / 'abi'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    header = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    out = (ctypes.c_int * 6)()
    _lib.lib().da_abi_sizes(out)
    binding = [ctypes.sizeof(c) for c in (_lib.WgradJob, _lib.ConvJob, _lib.WgradReduceDesc, _lib.RepackDesc,
                                          _lib.BnRunningDesc, _lib.BnPgradDesc)]
    assert header == list(out) == binding, (header, list(out), binding)


def _header_prototypes():
    """{name: (return type text, [parameter type texts])} of every function the public header declares: comments,
    preprocessor lines, the extern "C" braces and struct bodies stripped, one statement per ';'."""
    import re
    from deepards_amd import _lib
    txt = open(_lib.HEADER).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    txt = re.sub(r'//[^\n]*', ' ', txt)
    txt = re.sub(r'^\s*#[^\n]*$', ' ', txt, flags=re.M)
    txt = re.sub(r'extern\s+"C"\s*\{', ' ', txt)
    while True:                                                   # struct bodies (none is nested, the loop costs nothing)
        cut = re.sub(r'\{[^{}]*\}', ' ', txt)
        if cut == txt:
            break
        txt = cut
    protos = {}
    for stmt in txt.split(';'):
        stmt = ' '.join(stmt.replace('}', ' ').split())
        m = re.match(r'^(.*?)\b(da_[a-z0-9_]+)\s*\((.*)\)$', stmt)
        if not m or stmt.startswith('typedef'):
            continue
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in protos, 'declared twice: ' + name
        plist = [] if params in ('', 'void') else [p.strip() for p in params.split(',')]
        protos[name] = (ret, plist)
    return protos


def _c_class(decl, is_return=False):
    """A C declaration (parameter with its name, or a return type) -> ('ptr',) / ('void',) / ('int', bytes, signed) /
    ('float', bytes)."""
    import ctypes
    import re
    if '*' in decl or '[' in decl:
        return ('ptr',)
    words = [w for w in decl.split() if w != 'const']
    if not is_return:
        words = words[:-1]                                        # the parameter's name
    t = ' '.join(words)
    if t == 'da_stream_t':
        return ('ptr',)
    table = {'void': ('void',), 'int': ('int', 4, True), 'unsigned': ('int', 4, False), 'unsigned int': ('int', 4, False),
             'size_t': ('int', ctypes.sizeof(ctypes.c_size_t), False), 'long': ('int', ctypes.sizeof(ctypes.c_long), True),
             'long long': ('int', 8, True), 'int64_t': ('int', 8, True), 'float': ('float', 4), 'double': ('float', 8)}
    assert t in table, 'a type this check does not know: %r in %r' % (t, decl)
    assert re.match(r'^[A-Za-z_ ]+$', t)
    return table[t]


def _ctypes_class(c):
    """The same classes for a ctypes type (c_long and c_longlong are one class on LP64: size and signedness decide)."""
    import ctypes
    if c is None:
        return ('void',)
    if issubclass(c, (ctypes._Pointer, ctypes.Array)) or c in (ctypes.c_void_p, ctypes.c_char_p):
        return ('ptr',)
    code = c._type_
    if code in 'fd':
        return ('float', ctypes.sizeof(c))
    assert code in 'bhilqBHILQ', 'a ctypes class this check does not know: %r' % (c,)
    return ('int', ctypes.sizeof(c), code.islower())


def test_every_binding_matches_its_header_prototype():
    """_lib.SIGNATURES against include/deepards_hip.h, entry by entry: the return type and every parameter's class
    (pointer / da_stream_t <-> a pointer type; int, unsigned, size_t, long, float, double <-> the ctypes class of the same
    kind, size and signedness).  ctypes converts silently, so a size_t bound as c_int or a double bound as c_float would
    hand the library a wrong value without any error."""
    from deepards_amd import _lib
    protos = _header_prototypes()
    assert set(protos) == set(_lib.SIGNATURES)
    assert len(protos) >= 115
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = _lib.SIGNATURES[name]
        if _c_class(ret, is_return=True) != _ctypes_class(res):
            bad.append('%s: returns %r, bound as %r' % (name, ret, res))
        if len(params) != len(args):
            bad.append('%s: %d parameters in the header, %d bound' % (name, len(params), len(args)))
            continue
        for i, (p, a) in enumerate(zip(params, args)):
            if _c_class(p) != _ctypes_class(a):
                bad.append('%s: parameter %d %r bound as %r' % (name, i, p, a))
    assert not bad, '\n'.join(bad)


def test_product_path_refuses_cpu_tensors():
    import deepards_amd.models as M
    from deepards_amd import hip_ops as H
    model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        model(torch.zeros(2, 20, 1, 224), None)
    with pytest.raises(ValueError):
        H.bn_stats(torch.zeros(20, 56, 64), 20)
    # the product package never imports the oracle
    for name, mod in list(sys.modules.items()):
        if name.startswith('deepards_amd') and mod is not None:
            src = getattr(mod, '__file__', None)
            if src and src.endswith('.py'):
                assert 'oracle' not in open(src).read().replace('oracle/', '').replace('the oracle', ''), name


def test_model_surface_matches_reference_inventory():
    import deepards_amd.models as M
    from oracle.weights import param_spec
    for backbone, ctor, nkeys, nout in (('resnet18', M.resnet18, 129, 512), ('densenet18', M.densenet18, 64, 128)):
        bb = ctor()
        assert bb.network_name == backbone and bb.n_out_filters == nout
        model = M.CNNLinearNetwork(bb, 20, 0)
        assert model.seq_size == 224 and model.breath_block is bb
        assert tuple(model.linear_final.weight.shape) == (2, nout * 20)
        assert [n for n, _ in model.named_parameters()] == [s[0] for s in param_spec(backbone)]
        assert [tuple(p.shape) for _, p in model.named_parameters()] == [tuple(s[1]) for s in param_spec(backbone)]
        assert len(model.state_dict()) == nkeys
    d = M.densenet18()
    assert hasattr(d, 'features') and hasattr(d, 'avgpool') and hasattr(d, 'forward_no_pool')
    ks, st, pd = d.conv_info()
    assert len(ks) == len(st) == len(pd) == 24 and ks[:2] == [7, 3]
    assert all(not m.track_running_stats for m in d.modules() if isinstance(m, torch.nn.BatchNorm1d))
    assert M.base_networks['resnet18'] is M.resnet18
    with pytest.raises(Exception, match='sequence length of 224'):
        M.CNNLinearNetwork(M.resnet18(), 20, 0)(torch.zeros(1, 20, 1, 100), None)
    # reference init: conv ~ N(0, sqrt(2/(k*C_out))), BN gamma 1 / beta 0 (resnet.py:115-121)
    r = M.resnet18()
    w = r.layer3[0].conv1.weight
    assert abs(float(w.std()) - np.sqrt(2.0 / (3 * 256))) < 2e-3
    assert float(r.bn1.weight.min()) == 1.0 and float(r.bn1.bias.abs().max()) == 0.0


# Per Conv1d in module order, run-length coded ((wanted forward / data-gradient kernel, form of the step's batched repack,
# weight-gradient kernel of the float job on an even length -- None: never a conv_wgrad_multi job, more than 3 taps or a
# channel count off 32), repeat).  Recorded from the decision functions as they stood BEFORE they moved into one block
# (functional._is_wino / _step_pack_code and the ladder inside hip_ops.conv_wgrad_multi), not from the code under test.
_STEM3, _STEM1 = ((0, 0, None), 3), ((0, 0, None), 1)
_RESNET18_F32 = [_STEM3, ((4, 4, 4), 4)] + [((0, 0, 0), 1), ((4, 4, 4), 1), ((0, 0, 0), 1), ((4, 4, 4), 2)] * 2 + \
    [((0, 0, 0), 1), ((6, 6, 6), 1), ((0, 0, 0), 1), ((6, 6, 6), 2)]
_RESNET18_X3 = [_STEM3, ((49, 49, 4), 4)] + [((0, 49, 0), 1), ((49, 49, 4), 1), ((0, 49, 0), 1), ((49, 49, 4), 2)] * 2 + \
    [((0, 49, 0), 1), ((49, 49, 6), 1), ((0, 49, 0), 1), ((49, 49, 6), 2)]
_DENSENET18_WINO = [_STEM1] + ([((0, 0, 0), 1), ((4, 4, 0), 1)] * 2 + [((0, 0, 0), 1)]) * 4
_KERNEL_TABLE = {       # (backbone, conv dtype, storage dtype, DA_WINOGRAD)
    ('resnet18', 'f32', 'f32', True): _RESNET18_F32,
    ('resnet18', 'f32', 'f32', False): [_STEM3, ((0, 0, 0), 19)],
    ('resnet18', 'bf16', 'f32', True): [_STEM3, ((16, 16, 16), 19)],
    ('resnet18', 'bf16', 'bf16', True): [_STEM3, ((16, 16, 16), 19)],
    ('resnet18', 'f32x3p', 'f32', True): _RESNET18_X3,
    ('densenet18', 'f32', 'f32', True): _DENSENET18_WINO[:-1],
    ('densenet18', 'f32', 'f32', False): [_STEM1, ((0, 0, 0), 19)],
    ('densenet18', 'bf16', 'f32', True): _DENSENET18_WINO[:-1],
    ('densenet18', 'f32x3p', 'f32', True): _DENSENET18_WINO[:-1],
}


def test_kernel_choice_per_conv_is_pinned():
    """Which kernel every Conv1d of the two backbones runs on, under each arithmetic, equals the recorded table."""
    import deepards_amd.models as M
    from deepards_amd import functional as F, hip_ops as H
    assert (H.DIRECT, H.WINO2, H.WINO4, H.BF16, H.X3) == (0, 4, 6, 16, 49)      # da_repack_desc.points
    nets = {'resnet18': M.resnet18(), 'densenet18': M.densenet18()}
    old = (F.conv_dtype(), H.ACT, H.WINOGRAD_WGRAD, H.WGRAD_BF16)
    try:
        for (backbone, dtype, storage, wino), rle in sorted(_KERNEL_TABLE.items()):
            H.ACT = torch.float32
            F.set_conv_dtype(dtype)
            H.ACT = torch.bfloat16 if storage == 'bf16' else torch.float32     # (set_storage_dtype would call the library)
            H.WINOGRAD_WGRAD = wino
            got = []
            for m in nets[backbone].modules():
                if isinstance(m, torch.nn.Conv1d):
                    shape = tuple(m.weight.shape) + (m.stride[0], m.padding[0])
                    job = shape[2] <= 3 and shape[0] % 32 == 0 and shape[1] % 32 == 0
                    got.append((H.conv_kernel_wanted(*shape), H.step_pack_form(*shape), H.wgrad_kernel(*shape, 56) if job else None))
            assert got == [row for row, n in rle for _ in range(n)], (backbone, dtype, storage, wino)
    finally:
        H.ACT = torch.float32
        F.set_conv_dtype(old[0])
        H.ACT, H.WINOGRAD_WGRAD, H.WGRAD_BF16 = old[1:]


# The BatchNorm host queries on the (L, C) maps of the two backbones (windows of 20 rows: Wn = 20 L), per batch size
# W = 16, 64, 128.  _BN_GEOMETRY[target blocks][shape][batch] = (da_bn_mask_words / W -- the single-pass kernel's threads per
# window, da_bn_two_ok, da_bn_pool_ok(L)); _BN_CHUNKS[shape][batch] = (P, chunk) of da_bn_chunks.  Recorded from the library
# as it stood BEFORE the entry points' launch shapes moved into bn_single_pass_launch, not from the code under test.
_BN_SHAPES = [(112, 64), (56, 64), (56, 96), (56, 128), (28, 64), (28, 96), (28, 128), (14, 64), (14, 96), (14, 128), (14, 256),
              (7, 64), (7, 96), (7, 128), (7, 512)]
_BN_GEOMETRY = {
    256: [
        [(3584, 0, 0), (3584, 0, 0), (3584, 0, 0)],
        [(1792, 1, 0), (1792, 1, 0), (1792, 0, 0)],
        [(2688, 1, 0), (2688, 1, 0), (2688, 0, 0)],
        [(3584, 1, 0), (3584, 0, 0), (3584, 0, 0)],
        [(1024, 1, 0), (1024, 1, 0), (896, 1, 0)],
        [(1536, 1, 0), (1536, 1, 0), (1344, 1, 0)],
        [(2048, 1, 0), (1792, 1, 0), (1792, 1, 0)],
        [(512, 1, 0), (512, 1, 0), (512, 1, 0)],
        [(768, 1, 0), (768, 1, 0), (768, 1, 0)],
        [(1024, 1, 0), (1024, 1, 0), (1024, 1, 0)],
        [(2048, 1, 0), (2048, 1, 0), (2048, 1, 0)],
        [(256, 1, 1), (256, 1, 1), (256, 1, 1)],
        [(384, 1, 1), (384, 1, 1), (384, 1, 1)],
        [(512, 1, 1), (512, 1, 1), (512, 1, 1)],
        [(2048, 1, 1), (2048, 1, 1), (2048, 1, 1)],
    ],
    64: [
        [(3584, 0, 0), (3584, 0, 0), (3584, 0, 0)],
        [(1792, 1, 0), (1792, 0, 0), (1792, 0, 0)],
        [(2688, 1, 0), (2688, 0, 0), (2688, 0, 0)],
        [(3584, 0, 0), (3584, 0, 0), (3584, 0, 0)],
        [(1024, 1, 0), (896, 1, 0), (896, 1, 0)],
        [(1536, 1, 0), (1344, 1, 0), (1344, 1, 0)],
        [(1792, 1, 0), (1792, 1, 0), (1792, 1, 0)],
        [(512, 1, 0), (512, 1, 0), (512, 1, 0)],
        [(768, 1, 0), (768, 1, 0), (768, 1, 0)],
        [(1024, 1, 0), (1024, 1, 0), (1024, 1, 0)],
        [(2048, 1, 0), (2048, 1, 0), (2048, 1, 0)],
        [(256, 1, 1), (256, 1, 1), (256, 1, 1)],
        [(384, 1, 1), (384, 1, 1), (384, 1, 1)],
        [(512, 1, 1), (512, 1, 1), (512, 1, 1)],
        [(2048, 1, 1), (2048, 1, 1), (2048, 1, 1)],
    ],
    1024: [
        [(3584, 1, 0), (3584, 1, 0), (3584, 1, 0)],
        [(2048, 1, 0), (2048, 1, 0), (2048, 1, 0)],
        [(3072, 1, 0), (3072, 1, 0), (3072, 1, 0)],
        [(4096, 1, 0), (4096, 1, 0), (3584, 1, 0)],
        [(1024, 1, 0), (1024, 1, 0), (1024, 1, 0)],
        [(1536, 1, 0), (1536, 1, 0), (1536, 1, 0)],
        [(2048, 1, 0), (2048, 1, 0), (2048, 1, 0)],
        [(512, 1, 0), (512, 1, 0), (512, 1, 0)],
        [(768, 1, 0), (768, 1, 0), (768, 1, 0)],
        [(1024, 1, 0), (1024, 1, 0), (1024, 1, 0)],
        [(2048, 1, 0), (2048, 1, 0), (2048, 1, 0)],
        [(512, 1, 1), (512, 1, 1), (512, 1, 1)],
        [(768, 1, 1), (768, 1, 1), (768, 1, 1)],
        [(1024, 1, 1), (1024, 1, 1), (512, 1, 1)],
        [(4096, 1, 1), (2048, 1, 1), (2048, 1, 1)],
    ],
}
_BN_CHUNKS = [
    [(18, 128), (8, 288), (4, 576)],
    [(9, 128), (7, 160), (4, 288)],
    [(9, 128), (6, 192), (3, 384)],
    [(9, 128), (4, 288), (2, 576)],
    [(5, 128), (5, 128), (4, 160)],
    [(5, 128), (5, 128), (3, 192)],
    [(5, 128), (4, 160), (2, 288)],
    [(3, 96), (3, 96), (3, 96)],
    [(3, 96), (3, 96), (3, 96)],
    [(3, 96), (3, 96), (2, 160)],
    [(3, 96), (2, 160), (1, 288)],
    [(2, 96), (2, 96), (2, 96)],
    [(2, 96), (2, 96), (2, 96)],
    [(2, 96), (2, 96), (2, 96)],
    [(2, 96), (1, 160), (1, 160)],
]


def test_bn_geometry_per_backbone_shape_is_pinned():
    """The single-pass geometry, its predicates and the two-stage chunking answer what they answered before the BatchNorm
    host layer was folded onto one launch helper; forcing the two-stage kernels turns every single-pass form off."""
    import ctypes
    from deepards_amd import _lib
    lib = _lib.lib()
    try:
        for target, table in sorted(_BN_GEOMETRY.items()):
            assert lib.da_bn_debug_target_blocks(target) == 0
            for (L, C), row in zip(_BN_SHAPES, table):
                got = [(lib.da_bn_mask_words(W, 20 * L, C) // W, lib.da_bn_two_ok(W, 20 * L, C), lib.da_bn_pool_ok(W, 20 * L, C, L))
                       for W in (16, 64, 128)]
                assert got == row, (target, L, C, got)
                assert all(lib.da_bn_mask_words(W, 20 * L, C) % W == 0 for W in (16, 64, 128))
                assert not lib.da_bn_pool_ok(64, 20 * L, C, 3) and not lib.da_bn_pool_ok(64, 20 * L, C, 0)      # 3 does not divide 20 L
        assert lib.da_bn_debug_target_blocks(256) == 0 and lib.da_bn_debug_target_blocks(0) == -1
        for (L, C), row in zip(_BN_SHAPES, _BN_CHUNKS):
            for W, (P, chunk) in zip((16, 64, 128), row):
                gp, gc = ctypes.c_int(), ctypes.c_int()
                lib.da_bn_chunks(W, 20 * L, C, ctypes.byref(gp), ctypes.byref(gc))
                assert (gp.value, gc.value) == (P, chunk), (L, C, W)
                assert lib.da_bn_workspace(W, 20 * L, C) == 8 * W * C * P
        # no windows, no positions, or fewer channels than one channel group of 32: no geometry -- P = 0, chunk = 0 and no
        # workspace, answered without a signal (C < 32 used to divide by zero)
        for W, Wn, C in [(16, 1120, 0), (16, 1120, 1), (16, 1120, 16), (16, 1120, 31), (0, 1120, 64), (-1, 1120, 64),
                         (16, 0, 64), (16, -5, 64), (0, 0, 0)]:
            gp, gc = ctypes.c_int(-7), ctypes.c_int(-7)
            lib.da_bn_chunks(W, Wn, C, ctypes.byref(gp), ctypes.byref(gc))
            assert (gp.value, gc.value) == (0, 0), (W, Wn, C)
            assert lib.da_bn_workspace(W, Wn, C) == 0, (W, Wn, C)
        # ... and the entry points that launch over that geometry refuse such a shape before they launch anything
        buf = (ctypes.c_float * 64)()
        for C in (0, 16):
            assert lib.da_bn_stats_partial(buf, 32, 16, 1120, C, buf, None) == -1
            assert lib.da_bn_stats_merge(buf, 16, 1120, C, 1e-5, buf, buf, None) == -1
            assert lib.da_stem_stats_partial(buf, buf, 40, 20, 224, C, buf, None) == -1
        gp, gc = ctypes.c_int(), ctypes.c_int()
        lib.da_bn_chunks(1, 1, 32, ctypes.byref(gp), ctypes.byref(gc))          # the smallest shape that has one
        assert (gp.value, gc.value) == (1, 32) and lib.da_bn_workspace(1, 1, 32) == 8 * 32
        assert lib.da_bn_debug_two_stage(1) == 0
        for L, C in _BN_SHAPES:
            assert lib.da_bn_mask_words(64, 20 * L, C) == 0 and not lib.da_bn_two_ok(64, 20 * L, C) and not lib.da_bn_pool_ok(64, 20 * L, C, L)
    finally:
        lib.da_bn_debug_two_stage(0)
        lib.da_bn_debug_target_blocks(256)


def _wgrad_job(rows, L, N, C, k, code=0, stride=1, xform=False, dy_half=False):
    """A da_wgrad_job descriptor of Conv1d(C, N, k, stride, pad = k // 2) on rows x L outputs; the plan query dereferences
    nothing, so every operand is one dummy non-null address (the launch's pointer checks) and the workspace stays NULL."""
    from deepards_amd import _lib
    j = _lib.WgradJob()
    j.dy = j.x = 64
    j.rows, j.Lm, j.Ldy, j.lddy, j.N, j.Lx, j.ldx, j.C = rows, L, L // 2 if dy_half else L, N, N, L * stride, C, C
    j.dy_stride, j.dy_off, j.src_stride, j.ntaps = 1, 0, stride, k
    for t in range(k):
        j.src_off[t] = t - k // 2
    j.winograd = code
    if xform or dy_half:
        j.xform, j.dy_half, j.Wn, j.ldstat = 1, 1 if dy_half else 0, 20 * L, C
        j.mean = j.invstd = j.gamma = j.beta = 64
    return j


def _wgrad_slabs(jobs, chained):
    """-> (rc, [slabs per job]) of da_conv_wgrad_plan."""
    import ctypes
    from deepards_amd import _lib
    arr = (_lib.WgradJob * len(jobs))(*jobs)
    out = (ctypes.c_int * len(jobs))()
    rc = _lib.lib().da_conv_wgrad_plan(arr, len(jobs), chained, out)
    return rc, list(out)


def test_wgrad_plan_query_reports_what_the_launch_writes():
    """da_conv_wgrad_plan over job arrays (host only): the slab counts of the launch's own planning pass.
    Unchained, and chained below 8 dense-block jobs, a job's count is that job's alone (a direct job's = da_conv_wgrad_splits)
    whatever else the array holds; chained, 8 or more dense-block jobs are planned as a batch and the F(2,3) jobs behind the
    launch's last whole round of 1 024 slots write twice the slabs."""
    from deepards_amd import _lib
    _lib.build()
    lib = _lib.lib()

    def alone(j):
        return lib.da_conv_wgrad_splits(j.rows, j.Lm, j.N, j.C, j.ntaps)

    rows = 1280                                                  # B = 64 windows of 20 rows
    direct = [_wgrad_job(rows, 28, 128, 64, 3, stride=2), _wgrad_job(rows, 28, 128, 64, 1, stride=2),
              _wgrad_job(rows, 56, 64, 64, 3), _wgrad_job(rows, 7, 512, 256, 3, stride=2)]
    dense = [_wgrad_job(rows, 56, 128, 32 * (i + 1), 1, xform=True) for i in range(6)] + \
            [_wgrad_job(rows, 56, 32, 128, 3, xform=True), _wgrad_job(rows, 56, 128, 128, 1, dy_half=True)] * 3
    coded = [_wgrad_job(rows, 56, 64, 64, 3, code=1), _wgrad_job(rows, 7, 512, 512, 3, code=6),
             _wgrad_job(rows, 28, 128, 128, 3, code=16), _wgrad_job(rows, 14, 256, 128, 3, code=16, stride=2),
             _wgrad_job(rows, 14, 256, 256, 3, code=49), _wgrad_job(rows, 14, 256, 128, 1, code=49, stride=2)]
    # unchained: every job as if alone -- 12 dense-block jobs and all five winograd codes in one array, in two orders
    mixed = direct + dense + coded
    assert len(dense) == 12 and {j.winograd for j in mixed} == {0, 1, 6, 16, 49}
    # ... and chained with 7 dense-block jobs (one F(2,3) job: less than a round)
    for jobs, chained in ((mixed, 0), (mixed[::-1], 0), (coded + direct + dense[:7], 0), (coded + direct + dense[:7], 1)):
        rc, slabs = _wgrad_slabs(jobs, chained)
        assert rc == 0
        for j, s in zip(jobs, slabs):
            assert s >= 1 and _wgrad_slabs([j], 0) == (0, [s])
            if j.winograd == 0:
                assert s == alone(j)
    # chained, 8 or more dense-block jobs: the batch plan (per-job target 2560 // n blocks), not the job's plan alone
    big = _wgrad_job(2040, 56, 128, 64, 1, xform=True)           # M = 114 240 (B = 102)
    small = _wgrad_job(20, 56, 256, 512, 3, xform=True)          # M = 1 120
    assert (alone(big), alone(small)) == (255, 5)
    assert _wgrad_slabs([big] * 9, 1) == (0, [275] * 9)
    assert _wgrad_slabs([small] * 8, 1) == (0, [9] * 8)
    assert _wgrad_slabs([big] * 9, 0) == (0, [255] * 9) and _wgrad_slabs([small] * 7, 1) == (0, [5] * 7)
    assert lib.da_debug_set(7, 0) == 0                            # one launch per tile shape: no batch plan, here as in the launch
    try:
        assert _wgrad_slabs([big] * 9, 1) == (0, [255] * 9)
    finally:
        assert lib.da_debug_set(7, 1) == 0
    # chained F(2,3): resnet18 at B = 64, in the backward's order -- layer 3, layer 2 (1 008 blocks), layer 1 (224 blocks,
    # behind the last whole round of 1 024 slots: 448 half blocks, twice the slabs); the F(4,3) jobs are another launch
    wino = [_wgrad_job(rows, 7, 512, 512, 3, code=6)] * 3 + [_wgrad_job(rows, 14, 256, 256, 3, code=1)] * 3 + \
           [_wgrad_job(rows, 28, 128, 128, 3, code=1)] * 3 + [_wgrad_job(rows, 56, 64, 64, 3, code=1)] * 4
    rc, plain = _wgrad_slabs(wino, 0)
    assert rc == 0 and plain[3:] == [14] * 3 + [28] * 3 + [56] * 4
    blocks = [(j.N // 64) * (j.C // 64) * s for j, s in zip(wino, plain)]
    assert sum(blocks[3:9]) == 1008 and sum(blocks[9:]) == 224
    rc, chained = _wgrad_slabs(wino, 1)
    assert rc == 0 and chained == plain[:9] + [112] * 4
    assert sum((j.N // 64) * (j.C // 64) * s for j, s in zip(wino[9:], chained[9:])) == 448
    assert _wgrad_slabs(wino[:9], 1) == (0, plain[:9])          # 1 008 blocks: less than one round, as planned
    # jobs no kernel takes: DA_EINVAL from the query as from the launch
    for bad in (_wgrad_job(rows, 56, 32, 32, 3), _wgrad_job(rows, 56, 64, 64, 1, code=1), _wgrad_job(rows, 56, 96, 64, 3, code=6),
                _wgrad_job(rows, 56, 64, 64, 3, code=2), _wgrad_job(rows, 56, 64, 48, 1)):
        for chained in (0, 1):
            assert _wgrad_slabs([direct[0], bad], chained)[0] == -1
    assert _wgrad_slabs([], 0) == (0, [])


def test_host_helpers():
    from deepards_amd.train import clip_odd_batch_sizes, shard_windows
    idx, seq, meta, tgt = torch.arange(5), torch.zeros(5, 20, 1, 224), torch.zeros(5), torch.zeros(5, 2)
    a, b, c, d = clip_odd_batch_sizes(idx, seq, meta, tgt)
    assert a.shape[0] == b.shape[0] == c.shape[0] == d.shape[0] == 4
    a, b, c, d = clip_odd_batch_sizes(idx[:4], seq[:4], meta[:4], tgt[:4])
    assert b.shape[0] == 4
    assert shard_windows(64, 4, 1) == slice(16, 32)
    assert [shard_windows(8, 2, r) for r in range(2)] == [slice(0, 4), slice(4, 8)]
    with pytest.raises(ValueError):
        shard_windows(6, 4, 0)                       # untrimmed batches are a caller bug (epoch iterators trim first)


def test_epoch_batches_are_legal_for_every_world_size():
    """Every batch an epoch yields splits evenly over the ranks and keeps the reference's even-batch rule
    (train_ards_detector.py:146-147,482-494): N=70, batch 16, world 4 has a tail of 6 -> trimmed to 4 (1 per rank)
    instead of raising; the shards of a batch partition it."""
    from deepards_amd.train import _epoch_indices, shard_windows, legal_batch_len, batch_multiple

    class Store(object):
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n
    assert [batch_multiple(16, w) for w in (1, 2, 3, 4, 8)] == [2, 2, 6, 4, 8] and batch_multiple(1, 1) == 1
    assert legal_batch_len(6, 16, 4) == 4 and legal_batch_len(7, 16, 1) == 6 and legal_batch_len(1, 1, 1) == 1
    for n, bs in ((70, 16), (20, 6), (1000, 64), (9, 16)):
        for world in (1, 2, 4, 8):
            g = torch.Generator().manual_seed(3)
            seen = []
            for idx, _, _ in _epoch_indices(Store(n), bs, True, g, world):
                assert len(idx) % 2 == 0 and len(idx) % world == 0 and 0 < len(idx) <= bs
                parts = [idx[shard_windows(len(idx), world, r)] for r in range(world)]
                assert len({len(p) for p in parts}) == 1
                assert torch.equal(torch.cat(parts), idx)
                seen += idx.tolist()
            assert len(set(seen)) == len(seen)
            full, tail = divmod(n, bs)
            assert len(seen) == full * legal_batch_len(bs, bs, world) + legal_batch_len(tail, bs, world)
    sizes = [len(i) for i, _, _ in _epoch_indices(Store(70), 16, False, None, 4)]
    assert sizes == [16, 16, 16, 16, 4]
    with pytest.raises(ValueError):
        list(_epoch_indices(Store(10), 1, False, None, 2))


def test_capture_guard_holds_the_collector_off_and_restores_it():
    """deepards_amd.train._capture_graph: pending garbage is collected BEFORE the capture window opens, the cyclic
    collector is disabled inside it, and its previous state comes back afterwards -- also when the capture raises,
    and also when the collector was already off."""
    import contextlib
    import gc
    import weakref
    from deepards_amd.train import _capture_graph

    class Node(object):
        pass
    events = []

    @contextlib.contextmanager
    def fake_capture(graph):
        events.append(('enter', gc.isenabled(), ref() is None))
        yield
        events.append(('exit', gc.isenabled()))
    was = gc.isenabled()
    try:
        for state in (True, False):
            gc.enable() if state else gc.disable()
            n = Node()
            n.me = n
            ref = weakref.ref(n)
            del n                                              # cyclic garbage pending at the time of the capture
            events.clear()
            with _capture_graph(object(), _ctx=fake_capture):
                assert not gc.isenabled()
            assert events == [('enter', False, True), ('exit', False)]    # collected before the window, off inside
            assert gc.isenabled() == state
            with pytest.raises(KeyError):
                with _capture_graph(object(), _ctx=fake_capture):
                    raise KeyError('capture failed')
            assert gc.isenabled() == state
    finally:
        gc.enable() if was else gc.disable()


def _sync_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from deepards_amd.train import HotPathTrainer, shared_generator, _epoch_indices, shard_windows
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import deepards_amd.models as M
    torch.manual_seed(100 + rank)                              # every rank its own initialisation
    model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
    model.breath_block.bn1.running_mean.fill_(float(rank + 1))
    before = model.linear_final.weight.detach().clone()
    tr = HotPathTrainer(model, world_size=world, rank=rank)
    tr.sync_replicas()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()] +
                     [b.detach().reshape(-1).float() for b in model.buffers()])

    class Store(object):
        def __len__(self):
            return 70
    torch.manual_seed(5000 + 17 * rank)                        # ... and its own global RNG
    perms = []
    for gen in (None, torch.Generator().manual_seed(rank)):    # no generator / a different generator per rank
        g = shared_generator(tr, gen)
        perms.append(torch.cat([i[shard_windows(len(i), world, rank)] for i, _, _ in _epoch_indices(Store(), 16, True, g, world)]))
        full = torch.cat([i for i, _, _ in _epoch_indices(Store(), 16, True, shared_generator(tr, gen), world)])
        perms.append(full)
    q.put((rank, flat.numpy(), [p.numpy() for p in perms], bool(torch.equal(before, model.linear_final.weight))))
    dist.barrier()
    dist.destroy_process_group()


def test_replica_sync_and_shared_permutation_gloo_world2():
    """HotPathTrainer.sync_replicas + shared_generator over gloo, world 2 (the host side of config C4): ranks that
    were initialised differently hold rank 0's parameters AND buffers afterwards; with no seed / different seeds
    they still draw ONE permutation per epoch and shard it disjointly."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, f0, perms0, same0), (_, f1, perms1, same1) = res
    assert np.array_equal(f0, f1)                              # parameters and buffers identical after the sync
    assert same0 and not same1                                 # rank 0 kept its weights, rank 1 was overwritten
    for k in (0, 2):                                           # shards of one permutation: disjoint, equal sizes
        assert len(perms0[k]) == len(perms1[k]) and not set(perms0[k].tolist()) & set(perms1[k].tolist())
    for k in (1, 3):                                           # the full permutation every rank iterates is the same
        assert np.array_equal(perms0[k], perms1[k])
    assert not np.array_equal(perms0[1], perms0[3])            # a fresh seed per epoch


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from oracle import np_ref
    from oracle.weights import seeded_params, seeded_batch
    from deepards_amd.train import FlatBucket, shard_windows
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    params64 = {k: v.astype(np.float64) for k, v in seeded_params('densenet18', 0).items()}
    x, t = seeded_batch(world * 1, 20, 5)
    sl = shard_windows(x.shape[0], world, rank)
    out = np_ref.cnn_linear_forward_backward(params64, x[sl].astype(np.float64), t[sl].astype(np.float64),
                                             backbone='densenet18')
    names = sorted(out['grads'])
    tens = [torch.nn.Parameter(torch.from_numpy(params64[n].copy())) for n in names]
    for p, n in zip(tens, names):
        p.grad = torch.from_numpy(np.ascontiguousarray(out['grads'][n]))
    # FlatBucket is fp32 on the device of the params; here fp32 CPU
    tens32 = [torch.nn.Parameter(p.detach().float()) for p in tens]
    for p32, p in zip(tens32, tens):
        p32.grad = p.grad.float()
    bucket = FlatBucket(tens32)
    bucket.allreduce()
    gflat = (bucket.g / world).numpy().astype(np.float64)
    assert all(off % 64 == 0 for off in bucket.offsets)          # 256-B aligned segments
    # clamp AFTER the reduce, then the optimiser step -- identical on every rank
    newp, gs = [], []
    for n, p, off in zip(names, tens32, bucket.offsets):
        k = p.numel()
        gs.append(gflat[off:off + k])
        gi = np_ref.clamp_grad(gflat[off:off + k].reshape(p.shape), 0.01)
        pn, _ = np_ref.sgd_nesterov_step(params64[n], gi, None, first=True)
        newp.append(pn.ravel())
    q.put((rank, np.concatenate(gs), np.concatenate(newp), names))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_gloo_world2_matches_full_batch():
    """Sharding windows over 2 ranks + sum-all-reduce of the flat bucket + 1/W scale reproduces the
    full-batch gradient (BN never crosses windows; loss is a mean over equal shards)."""
    import torch.multiprocessing as mp
    from oracle import np_ref
    from oracle.weights import seeded_params, seeded_batch
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda r: r[0])
    (_, g0, p0, names), (_, g1, p1, _) = res
    assert np.array_equal(g0, g1) and np.array_equal(p0, p1)          # replicas stay bit-identical
    params64 = {k: v.astype(np.float64) for k, v in seeded_params('densenet18', 0).items()}
    x, t = seeded_batch(2, 20, 5)
    full = np_ref.cnn_linear_forward_backward(params64, x.astype(np.float64), t.astype(np.float64), backbone='densenet18')
    ref = np.concatenate([full['grads'][n].ravel() for n in names])
    assert np.abs(g0 - ref).max() < 1e-6 * (1 + np.abs(ref).max())


def _fold_group_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from deepards_amd.train import FlatBucket, HotPathTrainer, gather_fold_results, make_fold_groups, shared_generator
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    group, gworld, grank, folds = make_fold_groups(2, 5)               # 2 fold groups x 2 ranks, 5 folds (config C4's shape)
    # the gradient exchange stays inside the sub-group
    p = torch.nn.Parameter(torch.zeros(70))
    p.grad = torch.full((70,), float(rank + 1))
    bucket = FlatBucket([p])
    bucket.allreduce(group)
    # replica sync + one shared permutation per sub-group
    import deepards_amd.models as M
    torch.manual_seed(100 + rank)
    model = M.CNNLinearNetwork(M.densenet18(), 20, 0)
    tr = HotPathTrainer(model, world_size=gworld, rank=grank, process_group=group)
    tr.sync_replicas()
    w = model.linear_final.weight.detach().clone()
    torch.manual_seed(900 + rank)
    perm = torch.randperm(12, generator=shared_generator(tr, None))
    # checkpoint-time averaging of the replicas' running statistics inside the sub-group
    from deepards_amd.train import average_replica_buffers
    bn = torch.nn.BatchNorm1d(4)
    bn.running_mean.fill_(float(rank))
    bn.num_batches_tracked.fill_(7 + rank)
    average_replica_buffers(bn, gworld, group)
    avg = (float(bn.running_mean[0]), int(bn.num_batches_tracked))
    res = {(f, 1): {'votes': np.full((3, 2), 10 * f + grank)} for f in folds}
    merged = gather_fold_results(res, grank == 0)
    q.put((rank, gworld, grank, folds, float(bucket.g[0]), w.numpy(), perm.numpy(),
           sorted(merged), {k: int(v['votes'][0, 0]) for k, v in merged.items()}, avg))
    dist.barrier()
    dist.destroy_process_group()


def test_fold_groups_times_data_parallel_subgroups_gloo_world4():
    """BASELINE config C4's shape on the host side: 4 ranks as 2 fold groups x 2 data-parallel ranks
    (train.fold_group_layout / make_fold_groups, --fold-groups): folds dealt round-robin to the groups, the gradient
    all-reduce, the replica sync and the shared permutation stay inside a sub-group, and every rank ends with every fold's
    patient results (gather_fold_results takes them from the group leaders)."""
    import torch.multiprocessing as mp
    from deepards_amd.train import fold_group_layout
    assert fold_group_layout(4, 3, 2, 5) == ([[0, 1], [2, 3]], 1, [1, 3])
    assert fold_group_layout(4, 0, 1, 5)[2] == [0, 1, 2, 3, 4] and fold_group_layout(4, 2, 4, 5) == ([[0], [1], [2], [3]], 2, [2])
    with pytest.raises(ValueError):
        fold_group_layout(4, 0, 3, 5)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_fold_group_worker, args=(r, 4, port, q)) for r in range(4)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [(r[1], r[2]) for r in res] == [(2, 0), (2, 1), (2, 0), (2, 1)]
    assert [r[3] for r in res] == [[0, 2, 4], [0, 2, 4], [1, 3], [1, 3]]
    assert [r[4] for r in res] == [3.0, 3.0, 7.0, 7.0]                   # 1 + 2 and 3 + 4: sums within the sub-groups
    assert np.array_equal(res[0][5], res[1][5]) and np.array_equal(res[2][5], res[3][5])      # each group holds ITS leader's weights
    assert not np.array_equal(res[0][5], res[2][5])
    assert np.array_equal(res[0][6], res[1][6]) and np.array_equal(res[2][6], res[3][6])      # one permutation per group
    assert [r[9] for r in res] == [(0.5, 7), (0.5, 7), (2.5, 9), (2.5, 9)]   # running stats: group mean; counters: the leader's
    for r in res:                                                         # every rank: all five folds, the leaders' numbers
        assert r[7] == [(f, 1) for f in range(5)]
        assert r[8] == {(f, 1): 10 * f for f in range(5)}


def test_driver_mirror_names_and_no_cpu_path():
    """deepards_amd.train_ards_detector keeps the reference driver's names (train_ards_detector.py:45-69, 73-512,
    925-939, 1410-1436) and refuses to run without a GPU."""
    from deepards_amd import train_ards_detector as T
    assert set(T.network_map) <= {'cnn_lstm', 'cnn_linear', 'cnn_double_linear', 'cnn_single_breath_linear',
                                  'cnn_linear_compr_to_rf', 'cnn_linear_to_mean'}
    assert T.network_map['cnn_linear'] is T.CNNLinearModel and 'resnet18' in T.base_networks
    for name in ('run_train_epoch', 'handle_train_optimization', 'get_splits', 'train_and_test', 'get_base_network',
                 'get_optimizer', 'run_test_epoch', 'get_model', 'clip_odd_batch_sizes', 'set_loss_criterion',
                 'calc_loss', 'get_network', '_process_test_batch_results'):
        assert callable(getattr(T.CNNLinearModel, name)), name
    args = T.make_args()
    assert (args.network, args.base_network, args.batch_size, args.optimizer, args.learning_rate, args.n_sub_batches,
            args.weight_decay, args.clip_val, args.epochs) == ('cnn_linear', 'densenet18', 16, 'sgd', 0.001, 20, 0.0001,
                                                               0.01, 10)                      # defaults.yml
    with pytest.raises(TypeError):
        T.make_args(not_an_argument=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        T.CNNLinearModel(T.make_args(cuda=False))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            T.CNNLinearModel(T.make_args())


# The job rows (dst_stride, dst_off, src_stride, src_off, wtap, tap_split; ntaps = len(src_off)) the stride-2 wrappers handed
# to the library before they took them from one geometry function -- recorded from conv_fwd_multi / conv_fwd_bf16_s2 (forward
# pair: both give the same rows), conv_dgrad_s2_pair / conv_dgrad_bf16_s2_pair (odd problem, then the even one with two
# sources) and conv_dgrad / conv_dgrad_bf16_s2 (single convs: even positions, then odd).  The direct packs keep w's tap order,
# the bf16 packs come tap-reversed: the odd problem's source offsets are [1, 0] against [0, 1].
_S2_ROWS = {
    ('fwd', 3, False): [(1, 0, 2, [-1, 0, 1], [0, 1, 2], 0)],
    ('fwd', 1, False): [(1, 0, 2, [0], [0], 0)],
    ('fwd', 3, True): [(1, 0, 2, [-1, 0, 1], [0, 1, 2], 0)],
    ('fwd', 1, True): [(1, 0, 2, [0], [0], 0)],
    ('dgrad_pair', 3, False): [(2, 1, 1, [1, 0], [0, 2], 0), (2, 0, 1, [0, 0], [1, 0], 1)],
    ('dgrad_pair', 3, True): [(2, 1, 1, [0, 1], [0, 2], 0), (2, 0, 1, [0, 0], [1, 0], 1)],
    ('dgrad', 3, False): [(2, 0, 1, [0], [1], 0), (2, 1, 1, [1, 0], [0, 2], 0)],
    ('dgrad', 3, True): [(2, 0, 1, [0], [1], 0), (2, 1, 1, [0, 1], [0, 2], 0)],
    ('dgrad', 1, False): [(2, 0, 1, [0], [0], 0)],
    ('dgrad', 1, True): [(2, 0, 1, [0], [0], 0)],
}


def test_s2_entry_geometry_is_pinned():
    """The pure geometry function of a stride-2 block entry returns exactly the rows the wrappers spelled out one by one."""
    from deepards_amd import hip_ops as H
    for (form, k, rev), rows in sorted(_S2_ROWS.items()):
        got = H._s2_entry_rows(form, k, tap_reversed=rev)
        assert [tuple(r) for r in got] == rows, (form, k, rev, got)
        assert [len(r[3]) for r in got] == [len(r[3]) for r in rows]          # ntaps
        assert all(isinstance(v, int) for r in got for v in (r[0], r[1], r[2], r[5], *r[3], *r[4]))


def test_conv_entry_refusal_codes_are_pinned():
    """One refusal per distinct check of the convolution entry points (tests/tools/diff_conv_refusals.py holds the grid that
    was compared with the build before their argument fills were shared): DA_EINVAL before any launch, DA_OK for no rows."""
    import ctypes
    from deepards_amd import _lib
    lib = _lib.lib()
    P = 4096                                                    # a dummy non-null address; a refusal dereferences nothing
    E = -1

    def job(**kw):
        j = _lib.ConvJob()
        vals = dict(x=P, w=P, y=P, rows=40, Lm=28, Lsrc=56, ldx=64, C=64, Ldst=28, ldy=64, N=64, dst_stride=1, dst_off=0,
                    src_stride=2, ntaps=3, src_off=(-1, 0, 1), wtap=(0, 1, 2), accumulate=0, x2=None, w2=None, tap_split=0)
        vals.update(kw)
        for k, v in vals.items():
            if k in ('src_off', 'wtap'):
                for t in range(3):
                    getattr(j, k)[t] = v[t]
            else:
                setattr(j, k, v)
        return j

    def multi(fn, *jobs, n=None):
        return fn((_lib.ConvJob * len(jobs))(*jobs), len(jobs) if n is None else n, None)

    for wino in (lib.da_conv3_winograd, lib.da_conv3_winograd4):
        w = lambda rows=40, L=56, ldx=64, C=64, ldy=64, N=64, x=P: wino(x, P, P, rows, L, ldx, C, ldy, N, 0, None)
        assert w(x=None) == E and w(rows=-1) == E and w(L=0) == E and w(C=48, ldx=48) == E and w(N=48) == E and w(C=0) == E
        assert w(ldx=66) == E and w(ldx=32) == E and w(ldy=32) == E
        assert w(rows=0) == 0
        assert w(rows=1 << 20) == E                             # 32-bit element offsets
        assert w(rows=2, L=1 << 18) == E                        # tile units x units per row within 32 bits
    drop = lambda p=0.2, seed=P, part=P, R=20, rows=40, L=56: lib.da_conv3_winograd_drop(P, P, P, rows, L, 64, 64, 64, 64, seed, 7, p, part, R, None)
    assert drop(p=-0.1) == E and drop(p=1.0) == E and drop(seed=None) == E
    assert drop(R=0) == E and drop(R=3) == E and drop(R=2) == E  # records: whole windows of >= 64 pairs
    assert drop(rows=0) == 0
    bn = lambda R=20, pend=P, mean=P, C=64, p=0.2, rows=40: lib.da_conv3_winograd_bn(P, P, P, rows, 56, C, 64, 64, R, pend, mean, P, P, P, 1e-5,
                                                                                    P, 7, p, None, None)
    assert bn(pend=None) == E and bn(mean=None) == E and bn(C=160) == E and bn(R=1) == E and bn(R=3) == E and bn(p=1.0) == E
    assert bn(rows=0) == 0
    b = lambda rows=40, L=56, ldx=64, C=64, ldy=64, N=64, x=P: lib.da_conv3_bf16(x, P, P, rows, L, ldx, C, ldy, N, 0, None)
    assert b(x=None) == E and b(rows=-1) == E and b(L=0) == E and b(C=48, ldx=48) == E and b(N=32, ldy=32) == E and b(ldx=66) == E
    assert b(ldx=32) == E and b(ldy=32) == E and b(rows=0) == 0
    assert b(rows=1 << 16, L=1 << 15) == E and b(rows=(1 << 21) - 1, L=1 << 10, ldy=12800, N=12800) == E
    bb = lambda R=20, pend=P, mean=P, part=P, C=64, rows=40, L=56, N=64: lib.da_conv3_bf16_bn(P, P, P, rows, L, C, C, N, N, R, pend, mean, P, P, P,
                                                                                              1e-5, part, None)
    assert bb(N=32) == E and bb(R=0) == E and bb(R=3) == E and bb(R=2) == E and bb(pend=None, part=None) == E and bb(mean=None) == E
    assert bb(C=2048) == E and bb(rows=1 << 16, L=1 << 15) == E
    assert bb(rows=0) == 0 and bb(rows=0, R=0) == E
    so, wt = (ctypes.c_int * 3)(-1, 0, 1), (ctypes.c_int * 3)(0, 1, 2)
    g = lambda rows=40, Lm=28, ldx=64, C=64, N=64, ntaps=3, x=P: lib.da_conv_gemm(x, P, P, rows, Lm, 56, ldx, C, 28, 64, N, 1, 0, 2, ntaps, so, wt, 0, None)
    assert g(x=None) == E and g(rows=-1) == E and g(Lm=0) == E and g(ntaps=0) == E and g(ntaps=4) == E
    assert g(C=48) == E and g(N=48) == E and g(ldx=66) == E and g(rows=1, Lm=1 << 16) == E
    assert g(rows=0) == 0 and g(rows=0, C=48) == 0              # (no rows: answered in front of the shape checks)
    gm = lib.da_conv_gemm_multi
    assert gm(None, 1, None) == E and multi(gm, job(), n=0) == E and multi(gm, *[job(rows=0)] * 5) == E
    for kw in (dict(x=None), dict(rows=-1), dict(Lm=0), dict(ntaps=4), dict(C=48), dict(N=32), dict(N=96), dict(ldx=66),
               dict(rows=1, Lm=1 << 16, Lsrc=1 << 17, Ldst=1 << 16), dict(x2=P), dict(x2=P, w2=P, tap_split=0), dict(x2=P, w2=P, tap_split=3)):
        assert multi(gm, job(rows=0), job(**kw)) == E, kw
    assert multi(gm, job(rows=0), job(rows=0)) == 0
    bm = lib.da_conv_bf16_multi
    assert bm(None, 1, None) == E and multi(bm, job(), n=-1) == E and bm(None, 0, None) == 0
    for kw in (dict(x=None), dict(rows=-1), dict(Lm=0), dict(ntaps=4), dict(C=48), dict(C=0), dict(N=32), dict(ldx=66), dict(ldx=32),
               dict(ldy=32), dict(src_stride=3), dict(src_stride=1), dict(Lsrc=55), dict(dst_stride=0), dict(dst_off=-1),
               dict(dst_off=1), dict(Ldst=27), dict(wtap=(0, 1, 3)), dict(src_off=(-2, 0, 1)), dict(x2=P), dict(x2=P, w2=P, tap_split=3),
               dict(rows=1 << 16, Lm=1 << 15, Lsrc=1 << 16, Ldst=1 << 15), dict(rows=1 << 14, Lm=1 << 16, Lsrc=1 << 17, Ldst=1 << 16),
               dict(rows=1 << 12, Lm=1 << 10, Lsrc=1 << 11, Ldst=1 << 30)):
        assert multi(bm, job(rows=0), job(**kw)) == E, kw
    assert multi(bm, *[job(rows=0)] * 8, job(C=48)) == E        # more than 4 jobs: launches of 4, the ninth is still looked at
    assert multi(bm, *[job(rows=0)] * 9) == 0
    try:                                                        # bf16 activation storage: the fp32 kernels refuse
        assert lib.da_set_act_dtype(1) == 0
        assert lib.da_conv3_winograd(P, P, P, 40, 56, 64, 64, 64, 64, 0, None) == E
        assert lib.da_conv3_winograd4(P, P, P, 40, 56, 64, 64, 64, 64, 0, None) == E
        assert g() == E and multi(gm, job()) == E and g(rows=0) == E
    finally:
        lib.da_set_act_dtype(0)


class _OnGpu(object):
    """Stands in for a CUDA tensor as far as the wrappers' host checks look: a meta tensor that says it is on the GPU."""
    is_cuda = True

    def __init__(self, *shape, **kw):
        self.t = torch.empty(shape, device='meta', dtype=kw.get('dtype', torch.float32))

    def __getattr__(self, name):
        return getattr(self.t, name)

    def data_ptr(self):
        return 4096


def test_conv_wrappers_refuse_what_they_refused():
    """The shapes and out / accumulate combinations every conv wrapper of hip_ops refused before its checks moved into shared
    helpers still raise ValueError, in front of any library call (the operands have no memory)."""
    from deepards_amd import hip_ops as H
    T, bf = _OnGpu, torch.bfloat16
    x, x48 = T(4, 8, 64), T(4, 8, 48)
    x3 = T(4, 8, 4, 3, 16, dtype=bf)
    pk = T(2, 4, 18, 64, 8, dtype=bf)
    dy = T(4, 4, 128)
    cases = [
        # a CPU tensor is refused by every wrapper's first look
        lambda: H.conv3_winograd(torch.zeros(4, 8, 64), T(4, 64, 64)),
        lambda: H.conv3_x3p(torch.zeros(4, 8, 4, 3, 16, dtype=bf), pk),
        lambda: H.conv_fwd(x, T(3, 64, 32), 1, 1),
        lambda: H.conv_fwd(x48, T(3, 64, 48), 1, 1),
        lambda: H.conv_fwd(x, T(3, 64, 64), 1, 1, out=T(4, 7, 64)),
        lambda: H.conv3_winograd(x, T(5, 64, 64)),
        lambda: H.conv3_winograd(x, T(4, 64, 32)),
        lambda: H.conv3_winograd(x, T(4, 48, 64)),
        lambda: H.conv3_winograd(x, T(4, 64, 64), accumulate=True),
        lambda: H.conv3_winograd(x, T(4, 64, 64), out=T(4, 8, 32)),
        lambda: H.conv3_winograd(x, T(4, 64, 64), out=T(4, 64, 8).transpose(1, 2)),
        lambda: H.conv3_winograd(x, T(6, 64, 64), stats_R=2),
        lambda: H.conv3_winograd(x, T(4, 64, 64), out=T(4, 8, 64), accumulate=True, stats_R=2),
        lambda: H.conv3_bf16(x, T(1, 64, 64, dtype=bf)),
        lambda: H.conv3_bf16(x, T(3, 32, 64, dtype=bf)),
        lambda: H.conv3_bf16(x, T(3, 64, 32, dtype=bf)),
        lambda: H.conv3_bf16(x, T(3, 64, 64)),
        lambda: H.conv3_bf16(x, T(3, 64, 64, dtype=bf), accumulate=True),
        lambda: H.conv3_bf16(x, T(3, 64, 64, dtype=bf), out=T(4, 8, 128)),
        lambda: H.conv3_bf16_bn(x, T(3, 64, 64, dtype=bf), 3, want_records=True),
        lambda: H.conv3_bf16_bn(x, T(1, 64, 64, dtype=bf), 2, want_records=True),
        lambda: H.conv3_bf16_bn(x, T(3, 64, 64), 2, want_records=True),
        lambda: H.x3_merge(x),
        lambda: H.x3_merge(T(4, 8, 4, 3, 16)),
        lambda: H.conv3_x3p(x, pk),
        lambda: H.conv3_x3p(x3, T(2, 3, 18, 64, 8, dtype=bf)),
        lambda: H.conv3_x3p(x3, T(2, 4, 18, 64, 8)),
        lambda: H.conv3_x3p(x3, pk, accumulate=True),
        lambda: H.conv3_x3p(x3, pk, out=T(4, 8, 64)),
        lambda: H.conv3_x3p(x3, pk, out=T(4, 8, 128, dtype=bf)),
        lambda: H.conv3_x3p(x3, pk, out=T(4, 128, 8).transpose(1, 2)),
        lambda: H.conv_x3p_s2_fwd(x, pk, pk),
        lambda: H.conv_x3p_s2_fwd(T(4, 7, 4, 3, 16, dtype=bf), pk, pk),
        lambda: H.conv_x3p_s2_fwd(x3, pk, T(1, 4, 18, 64, 8, dtype=bf)),
        lambda: H.conv_x3p_s2_dgrad(x3, pk, x, pk),
        lambda: H.conv_x3p_s2_dgrad(x3, pk, T(4, 4, 4, 3, 16, dtype=bf), pk),
        lambda: H.conv_x3p_s2_dgrad(x3, pk, x3, pk, out=T(4, 16, 64)),
        lambda: H.conv_x3p_s2_dgrad(x3, pk, x3, pk, out=T(4, 16, 128, dtype=bf)),
        lambda: H.conv_fwd_bf16_s2(T(4, 7, 64), T(3, 128, 64, dtype=bf)),
        lambda: H.conv_fwd_bf16_s2(x),
        lambda: H.conv_fwd_bf16_s2(x, T(2, 128, 64, dtype=bf)),
        lambda: H.conv_fwd_bf16_s2(x, T(3, 128, 64)),
        lambda: H.conv_dgrad_bf16_s2(dy, T(3, 64, 128, dtype=bf), 9),
        lambda: H.conv_dgrad_bf16_s2(dy, T(3, 64, 128, dtype=bf), 8, accumulate=True),
        lambda: H.conv_dgrad_bf16_s2(dy, T(1, 64, 128, dtype=bf), 8, out=T(4, 8, 128)),
        lambda: H.conv_dgrad_bf16_s2(dy, T(3, 64, 64, dtype=bf), 8),
        lambda: H.conv_dgrad_bf16_s2_pair(dy, T(1, 64, 128, dtype=bf), dy, T(1, 64, 128, dtype=bf), 8),
        lambda: H.conv_dgrad_bf16_s2_pair(dy, T(3, 64, 128, dtype=bf), dy, T(1, 128, 128, dtype=bf), 8),
        lambda: H.conv_dgrad_bf16_s2_pair(dy, T(3, 64, 128, dtype=bf), T(4, 5, 128), T(1, 64, 128, dtype=bf), 8),
        lambda: H.conv_dgrad_bf16_s2_pair(dy, T(3, 64, 128, dtype=bf), dy, T(1, 64, 128, dtype=bf), 10),
        lambda: H.conv_dgrad(dy, T(3, 64, 64), 2, 1, 8),
        lambda: H.conv_dgrad(dy, T(3, 48, 128), 2, 1, 8),
        lambda: H.conv_dgrad(dy, T(3, 64, 128), 2, 1, 8, accumulate=True),
        lambda: H.conv_dgrad(dy, T(3, 64, 128), 2, 1, 8, out=T(4, 9, 64)),
        lambda: H.conv_fwd_multi([(x, T(3, 128, 32), 2, 1), (x, T(1, 128, 64), 2, 0)]),
        lambda: H.conv_fwd_multi([(x48, T(3, 128, 48), 2, 1)]),
        lambda: H.conv_wgrad(dy, x, 3, 2, 1, accumulate=True),
        lambda: H.conv_wgrad(dy, x, 3, 1, 1),
        lambda: H.conv_wgrad(dy, T(3, 8, 64), 3, 2, 1),
        lambda: H.conv_wgrad(T(4, 8, 128), x, 7, 1, 3, accumulate=True),
        lambda: H.conv_wgrad(T(4, 8, 128), x, 7, 1, 3, defer=True),
        lambda: H.wgrad_reduce_multi([((x, 2, 3, 128, 64), T(128, 64, 1))]),
        lambda: H.step_tail_multi([((x, 2, 3, 128, 64), T(64, 128, 3))], [], []),
    ]
    for n, call in enumerate(cases):
        with pytest.raises(ValueError):
            call()
            pytest.fail('case %d was accepted' % n)


def test_wgrad_padded_width_follows_the_instantiated_tile_pairs():
    """da_conv_wgrad_padded_n(N, C) -- the width hip_ops.conv_wgrad zero-pads dy's channels to -- asks wgrad_plan itself.
    Pinned here to the (output, input) tile pairs conv_wgrad_kernel is instantiated for (da_conv_wgrad's dispatch): the
    smallest multiple of 32 from N on that one of them divides together with C.  A pair added to or taken from the kernels
    fails this sweep instead of silently padding more, or refusing again."""
    from deepards_amd import _lib
    q = _lib.lib().da_conv_wgrad_padded_n
    pairs = [(128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (32, 128)]
    padded = 0
    for n in range(32, 545, 32):
        for c in range(32, 545, 32):
            want = next(m for m in range(n, n + 129, 32) if any(m % tn == 0 and c % tc == 0 for tn, tc in pairs))
            assert q(n, c) == want, (n, c, q(n, c), want)
            assert q(want, c) == want
            padded += want != n
    assert 0 < padded < 17 * 17
    assert (q(96, 64), q(224, 64), q(32, 32), q(160, 128), q(64, 96), q(512, 512)) == (128, 256, 128, 160, 128, 512)
    assert q(48, 64) == -1 and q(64, 48) == -1 and q(0, 64) == -1


class _StubBackbone(torch.nn.Module):
    """A breath block that only answers the fused head's questions: ``kind`` is what it reports for every sequence length, and
    handing anything over -- by the head-operand method or by forward_windows -- counts a run and raises TypeError('boom')."""
    n_out_filters = 4

    def __init__(self, kind):
        torch.nn.Module.__init__(self)
        self.kind, self.runs = kind, 0

    def head_operand_kind(self, seq_len):
        return self.kind

    def head_operand(self, x, rows_per_window):
        return self.forward_windows(x, rows_per_window, pooled=False)

    def forward_windows(self, x, rows_per_window, pooled=True):
        self.runs += 1
        raise TypeError('boom')


def test_fused_head_lets_a_type_error_from_the_backbone_through():
    import deepards_amd.models as M
    bb = _StubBackbone(M.HEAD_MAP)
    with pytest.raises(TypeError, match='boom'):
        M.CNNLinearNetwork(bb, 2, 0).forward_loss(torch.zeros(3, 2, 1, 224), torch.zeros(3, 2))
    assert bb.runs == 1


def test_fused_head_asks_before_the_backbone_runs():
    import deepards_amd.models as M
    bb = _StubBackbone(None)
    assert M.CNNLinearNetwork(bb, 2, 0).forward_loss(torch.zeros(3, 2, 1, 224), torch.zeros(3, 2)) is None
    assert bb.runs == 0


# name -> (BatchNorm keeps running statistics, keyword group of the driver's build arguments, bf16 storage under conv dtype
# bf16): what the name-prefix rules of the trainer, the driver and the checkpoint loader gave before the table took over
_BACKBONE_DATA = {
    'resnet18': (True, 'resnet_kwargs', True), 'resnet34': (True, 'resnet_kwargs', True),
    'densenet18': (False, 'densenet_kwargs', False), 'densenet121': (False, 'densenet_kwargs', False),
    'densenet169': (False, 'densenet_kwargs', False), 'densenet201': (False, 'densenet_kwargs', False),
    'se_resnet18': (True, None, False), 'se_resnet50': (True, None, False), 'se_resnet101': (True, None, False),
    'se_resnet152': (True, None, False), 'vgg11': (True, None, False), 'vgg13': (True, None, False),
}


def test_backbone_table_holds_what_the_name_prefixes_said():
    import deepards_amd.models as M
    assert set(M.base_networks) == set(_BACKBONE_DATA) == set(M.BACKBONES)
    for name in M.base_networks:
        factory, cls, group = M.BACKBONES[name]
        assert factory is M.base_networks[name] and cls is M.backbone_class(name) and issubclass(cls, M.Backbone), name
        assert (cls.running_stats, group, cls.bf16_storage) == _BACKBONE_DATA[name], name
    assert M.backbone_class('resnet50') is None
    for name in ('resnet18', 'densenet18', 'se_resnet18', 'vgg11'):              # the instance reads the same data
        bb = M.base_networks[name]()
        assert type(bb) is M.backbone_class(name)
        assert (bb.running_stats, bb.bf16_storage) == (_BACKBONE_DATA[name][0], _BACKBONE_DATA[name][2]), name
        assert not list(M.Backbone().state_dict()) and bb.head_operand_kind(224) == (M.HEAD_FLAT if name == 'vgg11' else M.HEAD_MAP)
        assert bb.head_operand_kind(256) == (M.HEAD_FLAT if name == 'vgg11' else None)


def test_driver_and_checkpoint_loader_build_through_one_function(monkeypatch, tmp_path):
    import deepards_amd.models as M
    from deepards_amd import checkpoint as C
    from deepards_amd import train_ards_detector as T
    calls = []

    def build(name, build_args=None):
        calls.append((name, build_args))
        return torch.nn.Linear(1, 1, bias=False)
    monkeypatch.setattr(M, 'build_base_network', build)
    drv = object.__new__(T.network_map['cnn_linear'])           # (the constructor needs a device; get_base_network does not)
    drv.args = T.make_args(base_network='se_resnet50')
    assert isinstance(drv.get_base_network(), torch.nn.Linear)
    assert calls == [('se_resnet50', drv._base_network_kwargs())]
    path = str(tmp_path / 'sd.pth')
    torch.save({'breath_block.weight': torch.full((1, 1), 3.0), 'linear_final.bias': torch.zeros(2)}, path)
    kw = {'base_network': 'vgg13', 'resnet_kwargs': {'initial_planes': 128}}
    net = C.load_base_network(path, M.base_networks, kw)
    assert calls[1:] == [('vgg13', kw)] and float(net.weight.detach()) == 3.0


def test_epoch_generator_seeds_are_pinned():
    """One seed formula for every family's epochs: seed + 1000 fold + epoch (+ 500009 for a test epoch, + 100003 (it + 1)
    for ProtoPNet's last-layer pass ``it``); no seed, no generator (torch's global RNG, like a DataLoader)."""
    import types
    from deepards_amd import train_ards_detector as T
    gen = T.BaseTraining._epoch_generator
    drv = types.SimpleNamespace(args=types.SimpleNamespace(seed=3))
    assert gen(drv, 1, 2).initial_seed() == 1005
    assert gen(drv, 1, 2, 500009).initial_seed() == 501014
    assert gen(drv, 1, 2, 100003 * (0 + 1)).initial_seed() == 101008
    drv.args.seed = None
    assert gen(drv, 1, 2) is None and gen(drv, 1, 2, 500009) is None
    for cls in (T.ProtoPNet1DModel, T.SiameseCNNLinearModel, T.AutoencoderModel, T.CNNLinearModel):
        assert cls._epoch_generator is gen and not hasattr(cls, '_generator')       # the families share the one formula
