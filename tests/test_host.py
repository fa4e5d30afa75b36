"""CPU-only host-logic tests: C-ABI exports, loader behaviour without a GPU, state bookkeeping,
training-step glue, config derivation, and the world_size-2 gradient reducer over gloo."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rvt_amd
from rvt_amd import _header, _lib, backbone_config
from rvt_amd.states import RNNStates, merge_mixed_batches
from rvt_amd.types import DataType, DatasetSamplingMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'rvt_hip.h')).read()
    return sorted(set(re.findall(r'\b(rvt_[a-z0-9_]+)\s*\(', hdr)))


def test_header_and_binding_agree():
    """An independent regex over the raw header against the names the binding derives from it."""
    assert declared_symbols() == _lib.EXPORTS == sorted(_lib._SIGS)


# ---- the header reader (rvt_amd/_header.py) on short synthetic headers: the exact ctypes types --------------------------------------
_VP, _I, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double


def _same_types(got, want):
    return len(got) == len(want) and all(a is b for a, b in zip(got, want))


def test_header_reader_prototypes():
    _, protos, _ = _header.parse('''
        /* a comment with ( and ; inside, int not_a_function(int x); and text right up to the end*/int rvt_a(const void* x,
                  float* y, int n,
                  float eps, void* stream);
        // a line comment (with a parenthesis; and a semicolon)
        #define RVT_SOMETHING {(int)sizeof(int), 0}
        const char* rvt_msg(void);
        double rvt_rate(float* scratch, int iters);
        size_t rvt_bytes(size_t n, long long slots, const long long* perm, const void* const* maps, const unsigned char* mask);
    ''')
    assert list(protos) == ['rvt_a', 'rvt_msg', 'rvt_rate', 'rvt_bytes']
    assert protos['rvt_a'].restype is _I and _same_types(protos['rvt_a'].argtypes, [_VP, _VP, _I, _F, _VP])
    assert protos['rvt_a'].argnames == ('x', 'y', 'n', 'eps', 'stream')
    assert protos['rvt_msg'].restype is ctypes.c_char_p and protos['rvt_msg'].argtypes == []
    assert protos['rvt_rate'].restype is _D and _same_types(protos['rvt_rate'].argtypes, [_VP, _I])
    assert protos['rvt_bytes'].restype is ctypes.c_size_t
    assert _same_types(protos['rvt_bytes'].argtypes, [ctypes.c_size_t, ctypes.c_longlong, _VP, _VP, _VP])


def test_header_reader_structs():
    structs, protos, enums = _header.parse('''
        #ifdef __cplusplus
        extern "C" {
        #endif
        enum { RVT_X = 0, RVT_Y = 1 };
        typedef struct Inner {
            int a, b;                       /* two names, one declarator */
            const float *w, *bias; const void* p; float eps;
        } Inner;
        typedef struct Outer {
            int struct_bytes;
            Inner by_value;
            const Inner* arr;               /* HOST array */
            void *y0, *x0;
            double* sums;
        } Outer;
        void rvt_fill(Outer* t);
        int rvt_use(const Outer* t, const Inner* i, int n);
        #ifdef __cplusplus
        }
        #endif
    ''')
    Inner, Outer = structs['Inner'], structs['Outer']
    assert enums == dict(RVT_X=0, RVT_Y=1)
    assert list(structs) == ['Inner', 'Outer'] and issubclass(Inner, ctypes.Structure) and issubclass(Outer, ctypes.Structure)
    assert [f for f, _ in Inner._fields_] == ['a', 'b', 'w', 'bias', 'p', 'eps'] == list(_header.fields(Inner))
    assert _same_types([t for _, t in Inner._fields_], [_I, _I, _VP, _VP, _VP, _F])
    assert [f for f, _ in Outer._fields_] == ['struct_bytes', 'by_value', 'arr', 'y0', 'x0', 'sums']
    assert _same_types([t for _, t in Outer._fields_], [_I, Inner, ctypes.POINTER(Inner), _VP, _VP, _VP])
    assert ctypes.sizeof(Outer) == 8 + ctypes.sizeof(Inner) + 4 * 8 and ctypes.sizeof(Inner) == 40
    # in a prototype a struct pointer is the very object c_void_p (callers pass byref), a void return is None
    assert protos['rvt_fill'].restype is None and _same_types(protos['rvt_fill'].argtypes, [_VP])
    assert protos['rvt_use'].restype is _I and _same_types(protos['rvt_use'].argtypes, [_VP, _VP, _I])


def test_header_reader_arrays_and_enums():
    text = '''
        enum { RVT_X = 0, RVT_Y = 1 };
        enum {                    /* one enumerator per line, a comment with a , and a = behind each */
            RVT_KIND_A = 3,       /* explicit */
            RVT_KIND_B,           /* auto-increment: 4 */
            RVT_KIND_C = -2,
            RVT_KIND_D            /* -1; no trailing comma */
        };
        enum { RVT_ELEMS = 1024, };
        typedef struct Row {
            const float* src; long long n;
            int d[5];
            int ky[4], kx [ 2 ];            /* two arrays, one declarator */
            unsigned block0;
            double w[3];
        } Row;
        int rvt_walk(const Row* rows, unsigned n, void* stream);
    '''
    structs, protos, enums = _header.parse(text)
    Row = structs['Row']
    assert [f for f, _ in Row._fields_] == ['src', 'n', 'd', 'ky', 'kx', 'block0', 'w']
    assert _same_types([t for _, t in Row._fields_], [_VP, ctypes.c_longlong, _I * 5, _I * 4, _I * 2, ctypes.c_uint, _D * 3])
    assert [getattr(Row, f).offset for f in _header.fields(Row)] == [0, 8, 16, 36, 52, 60, 64] and ctypes.sizeof(Row) == 88
    dt = np.dtype(Row)                       # what the device tables are built from
    assert dt.names == _header.fields(Row) and dt.itemsize == 88 and dt['d'].shape == (5,) and dt['kx'].shape == (2,)
    assert dt['src'] == np.dtype('<u8') and dt['block0'] == np.dtype('<u4') and dt['w'].base == np.dtype('<f8')
    assert _same_types(protos['rvt_walk'].argtypes, [_VP, ctypes.c_uint, _VP])
    assert enums == dict(RVT_X=0, RVT_Y=1, RVT_KIND_A=3, RVT_KIND_B=4, RVT_KIND_C=-2, RVT_KIND_D=-1, RVT_ELEMS=1024)


@pytest.mark.parametrize('text,says', [
    ('int rvt_a(const void* x, uint64_t n);', 'uint64_t'),                          # unknown type of a parameter
    ('typedef struct S { short a; } S;', 'short'),                                  # ... of a field
    ('int rvt_a(int n);\nstatic int counter = 0;\nint rvt_b(int n);', 'counter'),    # a declaration the reader has no rule for
    ('int rvt_a(int n);\nstruct Loose { int a; };', 'Loose'),                        # a struct outside the typedef form
    ('typedef struct S { int d[N]; } S;', r'd\[N\]'),                                # an array whose length is not a literal
    ('typedef struct S { int d[2][3]; } S;', r'd\[2\]\[3\]'),                        # more than one dimension
    ('typedef struct S { int d[]; } S;', r'd\[\]'),                                  # a flexible array member
    ('int rvt_a(int d[4], int n);', 'array in the prototype of rvt_a'),             # arrays are struct fields only
    ('enum { RVT_A = 1 << 2 };', '1 << 2'),                                         # an enumerator that is an expression
    ('enum { RVT_A = RVT_B };', 'RVT_B'),                                           # ... or another name
    ('enum { RVT_A, RVT_A };', 'RVT_A'),                                            # a name twice
    ('enum Kind { RVT_A = 0 };', 'Kind'),                                           # a named enum
], ids=['unknown_param_type', 'unknown_field_type', 'leftover_declaration', 'leftover_struct', 'array_symbolic_length', 'array_2d',
        'array_flexible', 'array_parameter', 'enum_expression', 'enum_alias', 'enum_duplicate', 'enum_named'])
def test_header_reader_refuses(text, says):
    with pytest.raises(RuntimeError, match=says):
        _header.parse(text)


def test_header_reader_names_a_missing_header(monkeypatch):
    monkeypatch.setattr(_header, 'HEADER_PATH', os.path.join(ROOT, 'include', 'no_such_header.h'))
    with pytest.raises(RuntimeError, match='no_such_header.h'):
        _header._read()


def test_derived_binding_covers_the_real_header():
    """Every prototype, the 7 host-side structs and the 5 device-table rows of include/rvt_hip.h; tuning.FIELDS is the struct's own order."""
    from rvt_amd import stage_driver, tuning
    assert set(_header.STRUCTS) == {'RvtTuning', 'RvtBlockWeights', 'RvtStageDesc', 'RvtStageRoutes', 'RvtBlockSaved', 'RvtBlockTrain',
                                    'RvtStageTrain'} | set(TABLE_ROWS)
    assert ('struct_bytes',) + tuning.FIELDS == _header.fields(tuning.RvtTuning) and tuning.RvtTuning is _header.STRUCTS['RvtTuning']
    assert all(getattr(stage_driver, n) is c for n, c in _header.STRUCTS.items() if n != 'RvtTuning' and n not in TABLE_ROWS)
    assert all(ty is ctypes.c_void_p or ty in (_I, _F, ctypes.c_size_t, ctypes.c_longlong) for sig in _lib._SIGS.values() for ty in sig)
    assert _lib._SIGS['rvt_stage_routes'][0] is ctypes.c_void_p and _lib._SIGS['rvt_stage_routes'][-1] is ctypes.c_void_p


# sizeof of the device-table rows and the descriptor kinds: the values the kernels' static_asserts and enum held before the header declared them
TABLE_ROWS = {'RvtPackDesc': 96, 'RvtLayerScaleDesc': 80, 'RvtOptimChunk': 40, 'RvtOptimGroup': 80, 'RvtEventStream': 48}
PACK_KINDS = {'RVT_PACK_COPY': 0, 'RVT_PACK_TRANSPOSE': 1, 'RVT_PACK_CONV_FWD': 2, 'RVT_PACK_CONV_DGRAD': 3, 'RVT_PACK_LSTM_ROWS': 4,
              'RVT_PACK_CONV_WGRAD_ACC': 5, 'RVT_PACK_CONV_DGRAD4': 6}


def test_table_rows_match_the_c_compiler(tmp_path):
    """The layout is pinned against a C compiler, not against the reader: a C99 program that includes the header prints sizeof, every
    offsetof and the enumerators; the ctypes structs, the numpy dtypes the tables are built from and ENUMS must say the same."""
    rows = {n: _header.STRUCTS[n] for n in TABLE_ROWS}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rvt_hip.h"', 'int main(void) {']
    for n, st in rows.items():
        lines.append(f'    printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f in _header.fields(st)]
    lines += [f'    printf("{e} %d\\n", (int){e});' for e in _header.ENUMS]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    for n, st in rows.items():
        dt = np.dtype(st)
        assert c[n] == ctypes.sizeof(st) == dt.itemsize == TABLE_ROWS[n], n
        assert dt.names == _header.fields(st)
        for f in dt.names:
            assert c[f'{n}.{f}'] == getattr(st, f).offset == dt.fields[f][1], (n, f)
    assert {e: c[e] for e in _header.ENUMS} == _header.ENUMS
    assert {e: c[e] for e in PACK_KINDS} == PACK_KINDS
    assert c['RVT_PACK_BLOCK_ELEMS'] == 1024 and c['RVT_OPTIM_CHUNK_ELEMS'] == 4096 and (c['RVT_F32'], c['RVT_BF16']) == (0, 1)
    # the offsets of the hand-written dtype this replaced (rvt_amd/weights.py: PACK_DT), and the formats numpy derives
    pk = np.dtype(rows['RvtPackDesc'])
    assert [pk.fields[f][1] for f in pk.names] == [0, 8, 16, 24, 32, 36, 40, 60, 76, 92]
    assert [pk[f].base.str for f in pk.names] == ['<u8', '<u8', '<u8', '<i8', '<i4', '<i4', '<i4', '<i4', '<i4', '<u4']
    assert (pk['d'].shape, pk['ky'].shape, pk['kx'].shape) == ((5,), (4,), (4,))


def test_launch_args_by_name_and_arity_guard():
    """A recorded launch is read by the header's parameter names; a record that does not fit the prototype raises and names the entry."""
    import opmodel
    args = (1, 2, None, 3, 0, 128, 64, 32, 0, None)          # rvt_linear_fwd(x, w, bias, y, dtype, M, N, K, gelu_in, stream)
    a = _header.LaunchArgs('rvt_linear_fwd', args)
    assert (a.M, a.N, a.K, a.dtype) == (128, 64, 32, 0) and a.has('x') and not a.has('bias') and not a.has('stream')
    with pytest.raises(TypeError, match="'M' is not a pointer parameter of rvt_linear_fwd"):
        a.has('M')
    with pytest.raises(AttributeError, match="rvt_linear_fwd has no parameter 'T_steps'"):
        a.T_steps
    assert opmodel.model('rvt_linear_fwd', args) == (2.0 * 128 * 64 * 32, (128 * (64 + 32) + 64 * 32) * 4.0)
    for fn in (_header.LaunchArgs, opmodel.model, opmodel.executed):
        with pytest.raises(TypeError, match='rvt_linear_fwd takes 10 arguments .* the record has 9'):
            fn('rvt_linear_fwd', args[:-1])
    with pytest.raises(TypeError, match='rvt_pack_table takes 5 arguments'):          # also an entry point that has no model
        opmodel.model('rvt_pack_table', (1, 2, 3, 0))


def test_generated_structs_are_accepted_by_the_library():
    """The C side compares struct_bytes with its own sizeof: the emulator build of the same header accepts the generated structs."""
    from rvt_amd import stage_driver as SD, tuning
    from tests.backends import emu_library
    from tests.test_route_record import _desc
    lib = emu_library()
    t = tuning.RvtTuning()
    t.struct_bytes = ctypes.sizeof(t)
    assert lib.rvt_get_tuning(ctypes.byref(t)) == 0, lib.rvt_last_error()
    t.struct_bytes -= 4
    assert lib.rvt_get_tuning(ctypes.byref(t)) != 0                     # (the guard is live)
    T = 1
    d, keep, B = _desc(torch.bfloat16, 32, T, 2560)
    assert d.struct_bytes == ctypes.sizeof(SD.RvtStageDesc)
    tr = SD.RvtStageTrain()
    assert lib.rvt_stage_routes(ctypes.byref(d), T, B, 1, 0, 0, ctypes.byref(tr.routes)) == 0, lib.rvt_last_error()
    saved = (SD.RvtBlockSaved * 2)()
    tr.saved = ctypes.cast(saved, ctypes.POINTER(SD.RvtBlockSaved))
    tr.struct_bytes = ctypes.sizeof(SD.RvtStageTrain)
    assert lib.rvt_stage_seq_bwd_ws_bytes(ctypes.byref(d), ctypes.byref(tr), T, B) > 0
    tr.struct_bytes += 8
    assert lib.rvt_stage_seq_bwd_ws_bytes(ctypes.byref(d), ctypes.byref(tr), T, B) == 0


def test_one_workspace_cache(monkeypatch):
    """One dict keyed (kind, device type, device index, stream): a buffer per kind, grow-only, the floor honoured, the dtype kept."""
    monkeypatch.setattr(_lib, '_WS', {})
    like = torch.zeros(1)
    st, a = _lib.workspace('wgrad', like, 10, torch.float32, floor=64)
    assert st is None and a.numel() == 64 and a.dtype == torch.float32
    assert _lib.workspace('wgrad', like, 64, torch.float32, floor=64)[1] is a          # fits: the same buffer
    b = _lib.workspace('wgrad', like, 65, torch.float32, floor=64)[1]
    assert b is not a and b.numel() == 65
    assert _lib.workspace('wgrad', like, 3, torch.float32, floor=64)[1] is b           # never shrunk
    c = _lib.workspace('fwd', like, 7, torch.uint8)[1]
    assert c.dtype == torch.uint8 and c.numel() == 7 and _lib.workspace('wgrad', like, 1, torch.float32)[1] is b      # kinds do not share
    assert sorted(_lib._WS) == [('fwd', 'cpu', None, 0), ('wgrad', 'cpu', None, 0)]


def test_one_status_check():
    class Lib:
        def rvt_last_error(self):
            return b'why'
    _lib.check('rvt_x', 0, Lib())
    with pytest.raises(RuntimeError, match='rvt_x failed: why'):
        _lib.check('rvt_x', 3, Lib())


def test_hip_library_loads_and_exports_every_symbol():
    """The gfx950 build must dlopen on a GPU-less host and export everything include/rvt_hip.h declares
    (no compute call is made)."""
    csrc = os.path.join(ROOT, 'rvt_amd', 'csrc')
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.hip', '.hpp'))] + [os.path.join(ROOT, 'include', 'rvt_hip.h')]
    if not os.path.exists(_lib.LIB_PATH) or any(os.path.getmtime(f) > os.path.getmtime(_lib.LIB_PATH) for f in srcs):
        subprocess.run(['bash', os.path.join(csrc, 'build.sh')], check=True, capture_output=True)
    lib = _lib.load_library()
    for sym in declared_symbols():
        assert hasattr(lib, sym), sym
    assert lib.rvt_is_emulator() == 0


# ---- the include graph of rvt_amd/csrc/*.hpp: kernel headers share code through helper headers, never through each other ----
# headers that define the model-side kernel families
KERNEL_HEADERS = {'mlp.hpp', 'mlp_chain.hpp', 'mlp_stream.hpp', 'dgrad_ln.hpp', 'ln_linear.hpp', 'attn_block.hpp', 'attn_core2.hpp',
                  'lstm_scan.hpp', 'lstm_scan2.hpp', 'lstm_scan3.hpp', 'stem.hpp', 'gemm.hpp', 'ppgemm.hpp', 'ppgemm_tn.hpp', 'rowops.hpp',
                  'bnact.hpp', 'events.hpp', 'pack.hpp'}
# kernel header -> kernel header edges that may exist, with the reason
ALLOWED_KERNEL_EDGES = {
    ('ppgemm_tn.hpp', 'ppgemm.hpp'): 'one engine in two contraction forms: PPGeom, PPMat, PPWork and the load stream are shared',
}
# headers that hold device helpers and no kernel; they include only each other
HELPER_HEADERS = {'common.hpp', 'lds_dma.hpp', 'opm.hpp', 'acc_frags.hpp', 'ln_pieces.hpp', 'fold.hpp', 'attn_pieces.hpp',
                  'line_bounce.hpp', 'gelu_lut.hpp'}
# ... except fold.hpp: its three split-K fold kernels are `static`, one copy per part of the library that includes the file
HELPER_KERNELS = {'fold.hpp': 3}
# the data-side families share through a family header by design (framecache / frames_*, evseq / evprep, optim / gradstats,
# simota / nms, augment*); host.hpp and gemm_host.hpp are host-side launch glue
OUT_OF_SCOPE = {'framecache.hpp', 'frames_augment.hpp', 'frames_gather.hpp', 'evseq.hpp', 'evprep.hpp', 'optim.hpp', 'gradstats.hpp',
                'simota.hpp', 'nms.hpp', 'augment.hpp', 'augment_map.hpp', 'cocoeval.hpp', 'host.hpp', 'gemm_host.hpp'}


def csrc_headers(csrc):
    """{header: (names of its #include "..." lines, number of lines that say __global__)}"""
    out = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith('.hpp'):
            with open(os.path.join(csrc, name)) as f:
                text = f.read()
            incs = [os.path.basename(i) for i in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, re.M)]
            out[name] = (incs, sum('__global__' in line for line in text.splitlines()))
    return out


def include_rule_violations(csrc):
    hdrs = csrc_headers(csrc)
    bad = []
    unsorted = set(hdrs) - KERNEL_HEADERS - HELPER_HEADERS - OUT_OF_SCOPE
    if unsorted:
        bad.append(f'headers in no list of this test: {sorted(unsorted)}')
    for gone in sorted((KERNEL_HEADERS | HELPER_HEADERS) - set(hdrs)):
        bad.append(f'{gone} is listed but does not exist')
    for name, (incs, n_kernels) in hdrs.items():
        if name in KERNEL_HEADERS:
            for inc in incs:
                if inc in KERNEL_HEADERS and (name, inc) not in ALLOWED_KERNEL_EDGES:
                    bad.append(f'{name} includes the kernel header {inc}: move what it needs into a helper header')
                elif inc not in KERNEL_HEADERS | HELPER_HEADERS and inc != 'rvt_hip.h':
                    bad.append(f'{name} includes {inc}, which is neither a kernel nor a helper header')
        elif name in HELPER_HEADERS:
            for inc in incs:
                if inc not in HELPER_HEADERS and inc != 'rvt_hip.h':
                    bad.append(f'helper header {name} includes {inc}')
            if n_kernels != HELPER_KERNELS.get(name, 0):
                bad.append(f'helper header {name} has {n_kernels} lines with __global__, expected {HELPER_KERNELS.get(name, 0)}')
    for (a, b) in ALLOWED_KERNEL_EDGES:
        if a in hdrs and b not in hdrs[a][0]:
            bad.append(f'allowed edge {a} -> {b} no longer exists: drop it from the list')
    return bad


def test_kernel_headers_include_helper_headers_only(tmp_path):
    """A kernel header never includes another kernel header (ALLOWED_KERNEL_EDGES apart), and a helper header defines no kernel
    (fold.hpp's three static ones apart): any kernel family can then be rewritten or retired without touching the others.
    Looks at #include "..." lines and at the one keyword only."""
    csrc = os.path.join(ROOT, 'rvt_amd', 'csrc')
    assert include_rule_violations(csrc) == []
    # the rule bites: the edge this layout was made to remove, put back in a copy
    for name in os.listdir(csrc):
        if name.endswith('.hpp'):
            with open(os.path.join(csrc, name)) as f:
                text = f.read()
            if name == 'attn_block.hpp':
                text = text.replace('#include "opm.hpp"', '#include "mlp.hpp"\n#include "opm.hpp"', 1)
            (tmp_path / name).write_text(text)
    assert include_rule_violations(str(tmp_path)) == ['attn_block.hpp includes the kernel header mlp.hpp: move what it needs into a helper header']


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the GPU-less failure mode')
def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback: with no GPU the package must raise, never silently compute elsewhere."""
    _lib._install_test_library(None)
    m = rvt_amd.RNNDetector(backbone_config('tiny', 'gen1'))
    x = torch.zeros(1, 20, 240, 304)
    with pytest.raises(RuntimeError, match='no CPU fallback|needs an AMD GPU|CUDA'):
        m(x)


def test_config_derivation_matches_reference_modifier():
    """config/modifier.py:28-41: Gen1 240x304 -> 256x320, partition (8,10); 1Mpx 360x640 -> 384x640, (6,10)."""
    g1 = backbone_config('tiny', 'gen1')
    assert tuple(g1.in_res_hw) == (256, 320) and tuple(g1.stage.attention.partition_size) == (8, 10)
    g4 = backbone_config('base', 'gen4')
    assert tuple(g4.in_res_hw) == (384, 640) and tuple(g4.stage.attention.partition_size) == (6, 10)
    assert backbone_config('small', 'gen1').stage.attention.dim_head == 24


def test_module_surface_matches_reference():
    m = rvt_amd.RNNDetector(backbone_config('base', 'gen4'))
    assert m.stage_dims == [64, 128, 256, 512] and m.strides == [4, 8, 16, 32] and m.num_stages == 4
    assert m.get_stage_dims((2, 3, 4)) == (128, 256, 512) and m.get_strides((2, 3, 4)) == (8, 16, 32)
    n_params = sum(p.numel() for p in m.parameters())
    assert n_params == 12_783_168 or abs(n_params - 12.78e6) < 0.02e6      # 12.78 M (Base backbone)
    sd = m.state_dict()
    assert 'stages.0.att_blocks.0.att_window.norm1.weight' not in sd          # Identity for the first window block
    assert 'stages.0.att_blocks.0.att_grid.norm1.weight' in sd
    assert tuple(sd['stages.3.lstm.conv1x1.weight'].shape) == (2048, 1024, 1, 1)
    assert float(sd['stages.1.att_blocks.0.att_grid.ls2.gamma'][0]) == pytest.approx(1e-5)
    with pytest.raises(AssertionError):
        m.get_stage_dims((0,))


def test_rnn_states_semantics():
    st = RNNStates()
    assert st.get_states(0) is None
    st.reset(0, torch.tensor([True, False]))            # no-op before first save
    h = torch.ones(2, 4, 3, 3, requires_grad=True) * 2
    c = torch.ones(2, 4, 3, 3)
    st.save_states_and_detach(0, [(h, c)] * 4)
    got = st.get_states(0)
    assert got[0][0].requires_grad is False
    assert st.get_states(1) is None
    st.reset(0, torch.tensor([True, False]))
    assert float(st.get_states(0)[0][0][0].abs().sum()) == 0 and float(st.get_states(0)[0][0][1].sum()) == 2 * 36
    st.reset(0, [1])
    assert float(st.get_states(0)[0][1].abs().sum()) == 0


def test_merge_mixed_batches():
    a = {'worker_id': 3, 'data': {DataType.EV_REPR: [torch.zeros(2, 1)], DataType.IS_FIRST_SAMPLE: torch.tensor([True, False])}}
    b = {'worker_id': 9, 'data': {DataType.EV_REPR: [torch.ones(1, 1)], DataType.IS_FIRST_SAMPLE: torch.tensor([True])}}
    out = merge_mixed_batches({DatasetSamplingMode.STREAM: a, DatasetSamplingMode.RANDOM: b})
    assert out['worker_id'] == 3
    assert out['data'][DataType.EV_REPR][0].shape == (3, 1)
    assert out['data'][DataType.IS_FIRST_SAMPLE].tolist() == [True, False, True]
    assert merge_mixed_batches(a) is a


REDUCER_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from rvt_amd.dist import StageGradReducer
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo')
red = StageGradReducer()
class M: pass
m = M(); red.attach(m)
torch.manual_seed(0)
ref = {s: torch.randn(5 * 3 + 7 + s) for s in range(4)}          # one flat fp32 bucket per stage
mine = {s: v * (rank + 1) for s, v in ref.items()}
ptrs = {s: v.data_ptr() for s, v in mine.items()}
for s in (3, 2, 1, 0):                     # backward order: stage 4 first
    m._stage_grad_hook(s, mine[s])
red.finish()
scale = sum(r + 1 for r in range(world)) / world
for s in range(4):
    assert torch.allclose(mine[s], ref[s] * scale, atol=1e-6), s
    assert mine[s].data_ptr() == ptrs[s]                          # reduced in place: the bucket IS the .grad storage
dist.destroy_process_group()
print('OK', rank)
'''


def test_stage_grad_reducer_world2_gloo(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text(REDUCER_WORKER)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                        '--master-addr', '127.0.0.1', '--master-port', '29731', str(script), ROOT],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('OK') == 2


DDP_BACKBONE_WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root)
from rvt_amd import _lib, tuning
tuning.use(**dict(tuning.TEST_GEOMETRY, gemm_resident=3))
from rvt_amd.dist import StageGradReducer
from tests.backends import emu_library
from tests.test_backbone import build_model
from tests import casegen
_lib._install_test_library(emu_library())          # CPU SIMT-emulator build of the HIP kernels (tests only)
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo')
torch.set_num_threads(2)
name = 'micro'
def run(model, seed, reducer):
    xs = torch.from_numpy(casegen.make_inputs(name, seed=seed))
    cots = [torch.from_numpy(a) for a in casegen.make_cotangents(name, seed=seed + 10)]
    feats, _ = model.forward_sequence(xs, None)
    model.zero_grad()
    torch.autograd.backward([feats[s + 1] for s in range(4)], cots)
    if reducer is not None:
        reducer.finish()
    return {k: p.grad.clone() for k, p in model.named_parameters()}
m = build_model(name, torch.device('cpu'), torch.float32)
red = StageGradReducer().attach(m)
mine = run(m, 100 + rank, red)                      # each rank: its own shard of sequences
m._stage_grad_hook = None
ref = [run(m, 100 + r, None) for r in range(world)]  # what every rank should end up with: the mean over shards
for k in mine:
    want = sum(g[k] for g in ref) / world
    err = (mine[k] - want).abs().max().item() / max(want.abs().max().item(), 1e-12)
    assert err < 1e-5, (k, err)
dist.destroy_process_group()
print('OK', rank)
'''


def test_backbone_data_parallel_world2_gloo(tmp_path):
    """Two processes, gloo, the real backward (HIP kernel sources on the CPU emulator): per-stage bucketed
    all-reduce launched from inside the stage-major backward must leave the mean gradient on every rank."""
    from tests.backends import emu_library
    emu_library()                                   # build once here, not concurrently in both workers
    script = tmp_path / 'ddp.py'
    script.write_text(DDP_BACKBONE_WORKER)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                        '--master-addr', '127.0.0.1', '--master-port', '29733', str(script), ROOT],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('OK') == 2


# ---- parameter-side tables, gradient buckets, grad-mode handling (CPU emulator build of the kernels) ----------------
def _emu_model(name='micro', dtype=torch.float32):
    from tests.backends import emu_library
    from tests.test_backbone import build_model
    _lib._install_test_library(emu_library())
    return build_model(name, torch.device('cpu'), dtype)


def test_pack_table_matches_reference_packings():
    """rvt_pack_table (one launch) == the plain tensor restatements of every packing (rvt_amd/weights.py)."""
    from rvt_amd import weights as Wt
    from tests import casegen
    try:
        for dtype in (torch.float32, torch.bfloat16):
            m = _emu_model('micro_dws_xh', dtype)
            xs = torch.from_numpy(casegen.make_inputs('micro_dws_xh'))
            m.forward_sequence(xs)                              # training-mode forward: builds + packs everything
            mw = m._mw_cache
            sd = {k: v.detach() for k, v in m.named_parameters()}
            for si, sw in enumerate(mw.stages):
                pre = f'stages.{si}.'
                g = m.stage_geoms(64, 96)[si]
                w = sd[pre + 'downsample_cf2cl.conv.weight']
                assert torch.equal(sw.conv_w, Wt.pack_conv_fwd(w, sw.cin_pad, dtype))
                if sw.conv_wd is not None:
                    assert torch.equal(sw.conv_wd, Wt.pack_conv_dgrad(w, g.stride, g.pad, dtype))
                wl = sd[pre + 'lstm.conv1x1.weight'].reshape(4 * g.C, 2 * g.C)
                perm = Wt.lstm_gate_perm(g.C, 'cpu')
                assert torch.equal(sw.lstm_w, wl[perm].to(dtype))
                assert torch.equal(sw.lstm_b, sd[pre + 'lstm.conv1x1.bias'][perm])
                assert torch.equal(sw.lstm_wn, wl.to(dtype)) and torch.equal(sw.lstm_wt, wl.t().to(dtype))
                bw = sw.blocks[0][1]
                bp = pre + 'att_blocks.0.att_grid.'
                assert torch.equal(bw['qkv_w'], sd[bp + 'self_attn.qkv.weight'].to(dtype))
                assert torch.equal(bw['fc1_wt'], sd[bp + 'mlp.net.0.0.weight'].t().to(dtype))
                want = (sd[bp + 'mlp.net.2.weight'] * sd[bp + 'ls2.gamma'][:, None]).t().to(dtype)
                assert torch.equal(bw['fc2_wt'], want)
                want = (sd[bp + 'self_attn.proj.weight'] * sd[bp + 'ls1.gamma'][:, None]).t().to(dtype)
                assert torch.equal(bw['proj_wt'], want)
    finally:
        _lib._install_test_library(None)


def test_no_grad_forward_takes_inference_path_and_weight_cache_tracks_parameters():
    from tests import casegen
    try:
        m = _emu_model()
        xs = torch.from_numpy(casegen.make_inputs('micro'))
        with torch.no_grad():
            f0, st = m.forward_sequence(xs)
        assert m._last_saved is None                             # nothing kept for a backward that cannot happen
        assert all(sw.lstm_wt is None for sw in m._mw_cache.stages)
        assert st[0][0]._base is None                            # states do not pin the (T+1)-slot feature buffer
        f1, _ = m.forward_sequence(xs)                           # grad mode on: training path, same numbers
        assert m._last_saved is not None
        for s in range(1, 5):
            assert torch.equal(f0[s], f1[s].detach())
        # in-place update through .data does not bump _version: inference must be told, training re-packs by itself
        p = m.stages[0].downsample_cf2cl.conv.weight
        with torch.no_grad():
            ref, _ = m.forward_sequence(xs)
            p.data.mul_(1.5)
            stale, _ = m.forward_sequence(xs)
            assert torch.equal(stale[1], ref[1])
            m.invalidate_weight_cache()
            fresh, _ = m.forward_sequence(xs)
            assert not torch.equal(fresh[1], ref[1])
            # .to()/param.data = ... replaces the storage: picked up without being told
            p.data = p.data.clone() * 2.0
            moved, _ = m.forward_sequence(xs)
            assert not torch.equal(moved[1], fresh[1])
    finally:
        _lib._install_test_library(None)


def test_gradient_buckets_accumulate_and_reassign():
    """.grad is a view of the stage's persistent bucket; a second backward without zeroing accumulates (like autograd),
    after zero_grad(set_to_none=True) the bucket restarts from zero, a foreign .grad tensor gets the result added."""
    from tests import casegen
    try:
        m = _emu_model()
        m.zero_copy_grads = True                                 # opt-in (bench.py, GraphedStep); the default is tested below
        xs = torch.from_numpy(casegen.make_inputs('micro'))
        cots = [torch.from_numpy(a) for a in casegen.make_cotangents('micro')]

        def bwd():
            feats, _ = m.forward_sequence(xs)
            torch.autograd.backward([feats[s + 1] for s in range(4)], cots)
        bwd()
        g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
        mw = m._mw_cache
        n0 = 'stages.2.att_blocks.0.att_grid.ls2.gamma'
        assert m.get_parameter(n0).grad.data_ptr() == mw.grads[2].g(n0).data_ptr()
        bwd()                                                    # accumulate
        for n, p in m.named_parameters():
            assert torch.allclose(p.grad, 2 * g1[n], rtol=1e-5, atol=1e-7 * float(g1[n].abs().max())), n
        m.zero_grad(set_to_none=True)
        bwd()
        for n, p in m.named_parameters():
            assert torch.equal(p.grad, g1[n]), n
        m.zero_grad(set_to_none=True)
        w = m.get_parameter(n0)
        w.grad = torch.ones_like(w)                              # foreign gradient tensor
        bwd()
        assert torch.allclose(w.grad, g1[n0] + 1.0)
        other = 'stages.2.att_blocks.0.att_grid.ls1.gamma'
        assert torch.equal(m.get_parameter(other).grad, g1[other])
    finally:
        _lib._install_test_library(None)


def test_default_gradient_handoff_obeys_autograd_contracts():
    """Default hand-off (no zero_copy_grads): gradients travel through autograd as tensors of their own - torch.autograd.grad
    returns them and leaves .grad alone, a .grad reference kept across steps is not overwritten by the next backward,
    accumulation without zeroing adds up."""
    from tests import casegen
    try:
        m = _emu_model()
        assert not getattr(m, 'zero_copy_grads', False)
        xs = torch.from_numpy(casegen.make_inputs('micro'))
        cots = [torch.from_numpy(a) for a in casegen.make_cotangents('micro')]
        names = [n for n, _ in m.named_parameters()]
        params = [p for _, p in m.named_parameters()]

        def loss():
            feats, _ = m.forward_sequence(xs)
            return sum((feats[s + 1] * cots[s]).sum() for s in range(4))
        got = torch.autograd.grad(loss(), params)
        assert all(g is not None for g in got) and all(p.grad is None for p in params)
        loss().backward()
        kept = {n: p.grad for n, p in zip(names, params)}
        snap = {n: g.clone() for n, g in kept.items()}
        mw = m._mw_cache
        for n, p in zip(names, params):
            assert torch.equal(p.grad, got[names.index(n)]), n
            assert p.grad.data_ptr() != mw.grads[int(n.split('.')[1])].g(n).data_ptr()      # not a view of the bucket
        m.zero_grad(set_to_none=True)
        (2.0 * loss()).backward()                                # a different gradient into the same buckets
        for n in names:
            assert torch.equal(kept[n], snap[n]), n              # the old reference still holds the old values
        loss().backward()                                        # accumulate on top of the 2x gradients
        for n, p in zip(names, params):
            assert torch.allclose(p.grad, 3.0 * snap[n], rtol=1e-5, atol=1e-6 * float(snap[n].abs().max())), n
    finally:
        _lib._install_test_library(None)


DROPIN_WORKER = r'''
# The drop-in claim of INTEGRATION.md section 1, executed: a detector with the reference YoloXDetector's layout (backbone / fpn /
# yolox_head, detector.py:18-41) whose three parts come from the registry branches a maintainer would add (INTEGRATION.md sections
# 1, 5 and 6) loads the reference detector's state_dict names strictly, and its forward_backbone over a short sequence with carried
# states, its detections, losses and feature gradients are compared with the reference's own detector, recorded with the same seeded
# weights and inputs in tests/golden/dropin_detector.npz (oracle/make_golden_dropin.py).
import os, sys
sys.dont_write_bytecode = True
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, 'oracle', '_stubs'))     # omegaconf stand-in (not installed here)
sys.path.insert(1, root)
import numpy as np
import torch
import torch.nn.functional as F
torch.set_num_threads(4)
from omegaconf import OmegaConf
import rvt_amd
from rvt_amd import _lib, tuning
from rvt_amd.fpn import build_yolox_fpn
from rvt_amd.head import build_yolox_head
from tests import casegen_dropin as cg
from tests.backends import emu_library
tuning.use(**tuning.TEST_GEOMETRY)
_lib._install_test_library(emu_library())          # CPU SIMT-emulator build of the HIP kernels (tests only)


class Detector(torch.nn.Module):
    # YoloXDetector's parts and calls, each part built by its `impl: mi355x` registry branch
    def __init__(self, cfg):
        super().__init__()
        assert cfg.backbone.name == 'MaxViTRNN' and cfg.backbone.get('impl', 'torch') == 'mi355x'
        self.backbone = rvt_amd.RNNDetector(cfg.backbone, compute_dtype=torch.float32)
        in_channels = self.backbone.get_stage_dims(cfg.fpn.in_stages)
        strides = self.backbone.get_strides(cfg.fpn.in_stages)
        self.fpn = build_yolox_fpn({k: v for k, v in cfg.fpn.items() if k != 'impl'}, in_channels, compute_dtype=torch.float32)
        self.yolox_head = build_yolox_head({k: v for k, v in cfg.head.items() if k != 'impl'}, in_channels, strides,
                                           compute_dtype=torch.float32)

    def forward_backbone(self, x, previous_states=None):
        return self.backbone(x, previous_states)

    def forward_detect(self, backbone_features, targets=None):
        fpn_features = self.fpn(backbone_features)
        if self.training:
            return self.yolox_head(fpn_features, targets)
        return self.yolox_head(fpn_features)


gold = np.load(os.path.join(root, 'tests', 'golden', cg.GOLDEN + '.npz'))
ours = Detector(OmegaConf.create(cg.model_cfg('mi355x'))).eval()
sd = ours.state_dict()
names = [str(n) for n in gold['names']]
assert sorted(sd) == sorted(names), 'state_dict names differ from the reference detector'
shapes = dict(zip(names, (str(x) for x in gold['shapes'])))
assert all(','.join(map(str, t.shape)) == shapes[n] for n, t in sd.items()), 'state_dict shapes differ from the reference detector'
assert [n for n in sd if n.startswith('fpn.')] == [n for n in names if n.startswith('fpn.')]   # OUR PAFPN, in the reference's order
ints = {n[4:]: gold[n] for n in gold.files if n.startswith('int:')}
missing = ours.load_state_dict(cg.seeded_state(sd, ints), strict=True)      # the WHOLE detector: backbone + FPN + head
assert not missing.missing_keys and not missing.unexpected_keys
assert type(ours.fpn).__module__.startswith('rvt_amd') and type(ours.yolox_head).__module__.startswith('rvt_amd')


def rel(a, ref):
    ref = torch.from_numpy(np.asarray(ref))
    assert tuple(a.shape) == tuple(ref.shape), (tuple(a.shape), tuple(ref.shape))
    return (a.detach().float() - ref).abs().max().item() / ref.abs().max().item()


xs = cg.make_inputs()
st_o = None
with torch.no_grad():
    for t in range(xs.shape[0]):
        fo, st_o = ours.forward_backbone(F.pad(xs[t].float(), [0, 6, 0, 4]), st_o)     # modules/detection.py:133-134
        assert sorted(fo) == [1, 2, 3, 4]
        for s in fo:
            err = rel(fo[s], gold[f'feat_t{t}_s{s}'])
            assert err < 1e-3, (t, s, err)
    for i, (ho, co) in enumerate(st_o):
        assert rel(ho, gold[f'h{i}']) < 1e-3 and rel(co, gold[f'c{i}']) <= 1e-3, i
    # OUR PAFPN + OUR head (HIP kernels, eval-mode BatchNorm) consume OUR features (eval: decoded predictions)
    out_o, _ = ours.forward_detect(backbone_features=fo)
    assert rel(out_o, gold['detections']) <= 2e-3
# training mode: targets -> OUR batched on-device SimOTA + losses against the reference's per-image loop (yolo_head.py:291-606) on the
# reference's own last-step features: same losses, same gradient into the backbone features
ours.train()
fo_g = {s: torch.from_numpy(gold[f'feat_t{xs.shape[0] - 1}_s{s}']).clone().requires_grad_(True) for s in (1, 2, 3, 4)}
_, loss_o = ours.forward_detect(backbone_features=fo_g, targets=cg.make_targets())
assert sorted(loss_o) == sorted(n[5:] for n in gold.files if n.startswith('loss:'))
for k in ('loss', 'iou_loss', 'conf_loss', 'cls_loss', 'num_fg'):
    a, b = float(loss_o[k]), float(gold['loss:' + k])
    assert abs(a - b) <= 2e-3 * max(abs(b), 1e-6), (k, a, b)
loss_o['loss'].backward()
for s in (2, 3, 4):
    err = rel(fo_g[s].grad, gold[f'feat_grad_s{s}'])
    assert err < 2e-3, (s, err)
print('DROPIN OK')
'''


def test_dropin_through_reference_registry_and_detector(tmp_path):
    """VERDICT r3 item 9 / SURVEY.md §8b: the drop-in claim, against the reference's own `YoloXDetector`
    (models/detection/yolox_extension/models/detector.py:18-41) as recorded in tests/golden/dropin_detector.npz, on the emulator library."""
    script = tmp_path / 'dropin.py'
    script.write_text(DROPIN_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'DROPIN OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it (the form the scaling run uses) must START two ranks under
    torch.distributed.run instead of asserting, and each rank must then fail loudly - with the device count in the message -
    when the box has fewer GPUs than ranks (this container: none).  No CPU fallback."""
    import subprocess
    import sys
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip('box has >= 2 GPUs: the launch would succeed (covered by the gpu-marked test)')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0',
                        '--workload', 'tiny_gen1', '--no-cpu-baseline'], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0
    assert 'launching 2 ranks under torch.distributed.run' in r.stderr, r.stderr[-2000:]
    assert 'AssertionError' not in r.stderr, r.stderr[-2000:]
    n_vis = torch.cuda.device_count()
    # every rank whose device is missing says so itself (rank 1 always; rank 0 too when there is no GPU at all)
    assert f'needs cuda:1 but only {n_vis} device(s) are visible' in r.stderr, r.stderr[-2000:]


def test_bench_rejects_mismatched_world_size():
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0',
                        '--no-cpu-baseline'], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and 'WORLD_SIZE=1' in r.stderr and 'AssertionError' not in r.stderr, r.stderr[-1500:]
