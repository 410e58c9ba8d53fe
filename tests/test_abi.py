"""The C-ABI library loads (no GPU needed) and exports every symbol include/recattend.h
declares; the ctypes table (ra_native.SIGNATURES), which ra_native derives from that header, covers
exactly that set, and a handful of its rows are pinned here literally."""
import ctypes
import os
import re

import pytest

import ra_native as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
  text = open(os.path.join(ROOT, 'include', 'recattend.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(ra_[a-z0-9_]+)\s*\(', text)))


def test_every_declared_symbol_is_exported():
  lib = ctypes.CDLL(rn.LIB_PATH)
  syms = _header_symbols()
  assert len(syms) >= 25
  for s in syms:
    assert hasattr(lib, s), s


def _header_abi_version():
  import re
  return int(re.search(r'#define RA_ABI_VERSION (\d+)', open(os.path.join(ROOT, 'include', 'recattend.h')).read()).group(1))


def test_binding_table_matches_header():
  assert sorted(rn.SIGNATURES) == _header_symbols()
  rn.lib()  # resolves them all
  assert rn.lib().ra_version() == rn.RA_ABI_VERSION == _header_abi_version()


_P, _I, _F, _Z, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_double
_DESC = ctypes.POINTER(rn.CtrlDesc)
# written out by hand from the header: between them every C type the reader maps (int, float, double, size_t, the data
# pointers incl. `const float *const *` and `unsigned short *`, const ra_ctrl_desc *, the char * return, a void argument list)
PINNED = {
    'ra_version': (_I, []),
    'ra_last_error_string': (ctypes.c_char_p, []),
    'ra_fill_f32': (_I, [_P, _Z, _F, _P]),
    'ra_hungarian_dev_workspace_bytes': (_Z, [_I, _I, _I]),
    'ra_bn_act_pool_bwd_dx_f32': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _D, _F, _I, _I, _I, _I, _I, _I, _P, _P]),
    'ra_bn_act_pool_bf16_f32': (_I, [_P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    'ra_ctrl_split_workspace_bytes': (_Z, [_DESC, _I]),
    'ra_ctrl_pack_weights': (_I, [_DESC, _P, _P, _P, _P]),
    'ra_controller_f32': (_I, [_DESC, _P, _P, _I, _P, _P, _P, _P, _P]),
    'ra_conv3x3_f32': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P]),
    'ra_conv3x3_plan': (_I, [_I] * 13 + [_P]),
    'ra_conv_pair_plan': (_I, [_I] * 10 + [_P]),
    'ra_conv_split_plan': (_I, [_I] * 7 + [_P]),
    'ra_conv_wino_plan': (_I, [_I] * 6 + [_P]),
    'ra_conv_pair_wino_plan': (_I, [_I] * 3 + [_P]),
    'ra_paste_plan': (_I, [_I] * 10 + [_Z, _I, _P]),
}


def test_pinned_signatures():
  for name, sig in PINNED.items():
    assert rn.SIGNATURES[name] == sig, name
  fn = rn.lib().ra_bn_act_pool_bwd_dx_f32
  assert fn.restype is _I and list(fn.argtypes) == PINNED['ra_bn_act_pool_bwd_dx_f32'][1]


def test_header_constants_and_descriptor():
  assert (rn.RA_E_INVALID, rn.RA_E_SHAPE, rn.RA_E_WORKSPACE) == (-1, -2, -3)
  assert rn.RA_CONV_TRANSPOSED == 1 and rn.RA_ATTN_STRIDE == 16
  assert [n for n, _ in rn.CtrlDesc._fields_] == ['G', 'Cf', 'hid', 'iters', 'n_gmlp', 'n_cmlp', 'mlp_dim', 'H', 'W', 'Fh', 'Fw',
                                                  'squash', 'fixed_var', 'dynamic_var', 'fixed_gamma']
  assert all(t is ctypes.c_int for _, t in rn.CtrlDesc._fields_) and ctypes.sizeof(rn.CtrlDesc) == 15 * 4


_SYNTHETIC = """
#define RA_SEVEN 7
#define RA_MINUS (-3) /* in parentheses */
typedef struct ra_ctrl_desc { int G; int H, W; } ra_ctrl_desc;
/* a comment with a call in it: ra_ghost(int x); */
size_t ra_good(const ra_ctrl_desc *d, const float *const *w /*[n]*/, unsigned short *h, double x, float y);
%s
"""


def test_reader_is_strict():
  sigs, consts, fields = rn.read_header(_SYNTHETIC % 'int ra_none(void);')
  assert sigs == {'ra_good': (_Z, [_DESC, _P, _P, _D, _F]), 'ra_none': (_I, [])}
  assert consts == {'RA_SEVEN': 7, 'RA_MINUS': -3} and fields == ['G', 'H', 'W']
  for bad, named in (('int ra_bad_arg(long n);', 'ra_bad_arg'),            # a type without a mapping
                     ('long ra_bad_ret(int n);', 'ra_bad_ret'),
                     ('int ra_bad_ptr(ra_other *p);', 'ra_bad_ptr'),
                     ('int ra_callback(int (*fn)(int), int n);', 'ra_callback'),  # prototypes it cannot split
                     ('int ra_unnamed(int, float *);', 'ra_unnamed'),
                     ('int ra_array(int v[4]);', 'ra_array'),
                     ('int ra_no_parens;', 'ra_no_parens')):
    with pytest.raises(rn.RecAttendError) as e:
      rn.read_header(_SYNTHETIC % bad)
    assert named in str(e.value), bad
  with pytest.raises(rn.RecAttendError):
    rn.read_header('int ra_x(void);')  # no struct ra_ctrl_desc


def test_argument_validation_without_gpu():
  lib = rn.lib()
  assert lib.ra_conv_cout_padded(1) == 16 and lib.ra_conv_cout_padded(96) == 128
  assert lib.ra_conv_cout_padded(129) == 0
  assert lib.ra_conv_packed_floats(6, 8) == 0          # Cin % 4
  assert lib.ra_conv_packed_floats(8, 8) == 9 * 8 * 16
  # null pointers are rejected before any launch
  rc = lib.ra_conv3x3_f32(None, 4, None, 0, 1, 8, 8, 0, None, None, None, 8, 1, 1, None, -1, None, None)
  assert rc == -1 and b'bad argument' in lib.ra_last_error_string()
  rc = lib.ra_hungarian_f32(None, 1, 2, 2, None, None, None)
  assert rc == -1
  assert lib.ra_resample_bwd_workspace_floats(8, 48, 4) == 8 * 48 * 8 and lib.ra_ctrl_train_supported(256, 64, 256, 5, 9) == 1


def test_plan_queries_without_gpu():
  """The launch-plan queries are host code: K1's whole plan and the pair's geometry need no device, the launch's own argument
  checks answer a bad shape, and nothing is written but the record."""
  lib = rn.lib()
  assert rn.RA_PLAN_INTS >= 21 and len({v for k, v in rn.CONSTANTS.items() if k.startswith('RA_PLAN_') and not k.startswith(
      ('RA_PLAN_FAMILY_', 'RA_PLAN_FORM_', 'RA_PLAN_INTS'))}) == 21  # the record's indices are distinct
  rec = (ctypes.c_int * rn.RA_PLAN_INTS)()
  # 16 -> 32 channels, 128 images of 18 x 50, pool 2: 512 workgroups of the 32 x 16 tile, two cout groups per wave, plain stores
  assert lib.ra_conv3x3_plan(16, 0, 128, 18, 50, 0, 3, 32, 2, 0, 0, 0, 0, rec) == 0
  got = {k: rec[getattr(rn, 'RA_PLAN_' + k)] for k in ('FAMILY', 'FORM', 'CK', 'NC', 'WN', 'GX', 'GY', 'KF', 'TILE_H', 'TILE_W', 'NTILES')}
  assert got == dict(FAMILY=rn.RA_PLAN_FAMILY_K1, FORM=0, CK=16, NC=2, WN=1, GX=4, GY=2, KF=3, TILE_H=16, TILE_W=32, NTILES=512), got
  assert lib.ra_conv3x3_plan(16, 0, 128, 18, 50, 0, 3, 32, 1, 0, 0, 0, 0, rec) == 0 and rec[rn.RA_PLAN_FORM] == rn.RA_PLAN_FORM_SWAP
  assert lib.ra_conv3x3_plan(6, 0, 1, 8, 8, 0, 3, 8, 1, 0, 0, 0, 0, rec) == rn.RA_E_SHAPE       # C0 % 4, as the launch answers
  assert lib.ra_conv3x3_plan(8, 0, 1, 8, 8, 0, 4, 8, 1, 0, 0, 0, 0, rec) == rn.RA_E_SHAPE       # filter size 4
  assert lib.ra_conv3x3_plan(8, 0, 1, 8, 8, 0, 3, 8, 1, 0, 0, 0, 0, None) == rn.RA_E_INVALID
  # the N-packed pair: 900 tiles on its 768 workgroups, XCD-contiguous, one or two tiles each
  assert lib.ra_conv_pair_plan(4, 225, 18, 34, 0, 8, 8, 2, 0, 0, rec) == 0
  assert rec[rn.RA_PLAN_FAMILY] == rn.RA_PLAN_FAMILY_PAIR and rec[rn.RA_PLAN_FORM] == rn.RA_PLAN_FORM_NPACKED
  assert [rec[i] for i in (rn.RA_PLAN_NTILES, rn.RA_PLAN_GRID, rn.RA_PLAN_TILES_MIN, rn.RA_PLAN_TILES_MAX, rn.RA_PLAN_XCD_MAP)] == [900, 768, 1, 2, 1]
  assert lib.ra_conv_pair_plan(4, 1, 16, 16, 0, 12, 8, 2, 0, 0, rec) == rn.RA_E_SHAPE           # CoutA 12
  # the paste: the decode loop's launch (canvas plane, one-channel patch) takes the window kernel, 4 rows per workgroup; a
  # packed patch channel, an image-channel canvas or a misaligned y_out the general one
  prec = (ctypes.c_int * rn.RA_PASTE_PLAN_INTS)()
  fields = (rn.RA_PASTE_PLAN_KERNEL, rn.RA_PASTE_PLAN_ROWS, rn.RA_PASTE_PLAN_GRID_X, rn.RA_PASTE_PLAN_THREADS, rn.RA_PASTE_PLAN_LDS)
  assert len(set(fields)) == 5 and max(fields) < rn.RA_PASTE_PLAN_INTS
  assert lib.ra_paste_plan(0, 8, 128, 128, 48, 48, 1, 0, 1, 0, 128 * 128, 1, prec) == 0
  assert [prec[i] for i in fields] == [rn.RA_PASTE_KERNEL_WINDOW, 4, 32, 256, 4 * 256 * 16 + (4 * 48 + 48 * 48 + 16) * 4]
  for args in ((0, 8, 128, 128, 48, 48, 4, 2, 1, 0, 128 * 128, 1), (0, 8, 128, 128, 48, 48, 1, 0, 0, 1, 128 * 128, 1),
               (0, 8, 128, 128, 48, 48, 1, 0, 1, 0, 128 * 128, 0), (1, 8, 126, 130, 48, 48, 1, 0, 0, 0, 126 * 130, 1)):
    assert lib.ra_paste_plan(*args, prec) == 0
    assert [prec[i] for i in fields] == [rn.RA_PASTE_KERNEL_GENERAL, 4, (args[2] + 3) // 4, 256, 4 * 48 * 4], args
  assert lib.ra_paste_plan(1, 8, 126, 128, 48, 48, 0, 0, 0, 0, 126 * 128, 1, prec) == 0 and prec[rn.RA_PASTE_PLAN_GRID_X] == 32
  assert prec[rn.RA_PASTE_PLAN_KERNEL] == rn.RA_PASTE_KERNEL_WINDOW                            # the box ignores Cp / pc
  assert lib.ra_paste_plan(0, 8, 128, 128, 48, 48, 1, 1, 1, 0, 128 * 128, 1, prec) == rn.RA_E_INVALID   # pc >= Cp, as the launch answers
  assert lib.ra_paste_plan(2, 8, 128, 128, 48, 48, 1, 0, 1, 0, 128 * 128, 1, prec) == rn.RA_E_INVALID
  assert lib.ra_paste_plan(0, 8, 128, 128, 48, 48, 1, 0, 1, 0, 128 * 128, 1, None) == rn.RA_E_INVALID


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
  monkeypatch.setattr(rn, 'LIB_PATH', str(tmp_path / 'nope.so'))
  monkeypatch.setattr(rn, '_lib', None)
  try:
    rn.lib()
    raise AssertionError('expected RecAttendError')
  except rn.RecAttendError as e:
    assert 'no CPU fallback' in str(e)
  finally:
    monkeypatch.undo()  # restores LIB_PATH and the loaded handle; reloading the module would fork
                        # RecAttendError into two classes for everything imported before
