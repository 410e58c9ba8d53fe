"""ctypes binding of librecattend.so (the C ABI declared in include/recattend.h).

There is NO fallback: if the shared library is missing or a symbol is absent the import
of the product path fails loudly.  Device pointers are taken from torch tensors
(`tensor.data_ptr()`), the stream from `torch.cuda.current_stream()`; torch is plumbing
(memory + streams) only.
"""
import ctypes as C
import os
import re

# The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES hardware queues
# (default 4, the null stream and the graph-capture stream included) and reads the variable at its
# first HIP call.  full_model.DecodePipeline keeps 4 batches in flight on 4 streams; two of them on one
# queue serialise (3.9 instead of 3.1 ms per cfg2 batch), so ask for 8 unless the user chose.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'librecattend.so')

HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'recattend.h')


class RecAttendError(RuntimeError):
  pass


class CtrlDesc(C.Structure):
  """struct ra_ctrl_desc; its _fields_ are read from the header below."""


class ImageGeo(C.Structure):
  """struct ra_image_geo, one image of a ragged batch; its _fields_ are read from the header below."""


_SCALARS = {'int': C.c_int, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t}
_POINTEES = ('float', 'int', 'void', 'unsigned short', 'double', 'unsigned char', 'unsigned long long', 'short', 'ra_image_geo',
             'unsigned int')
_MEMBERS = {'int': C.c_int, 'long long': C.c_longlong}


def _ctype(words, name):
  """ctypes type of a C type given as its tokens (`const` dropped): a scalar, ra_ctrl_desc *, or any other data pointer."""
  if words == ['ra_ctrl_desc', '*']:
    return C.POINTER(CtrlDesc)
  base = ' '.join(w for w in words if w != '*')
  if '*' in words and words[-1] == '*' and base in _POINTEES:
    return C.c_void_p
  if len(words) == 1 and base in _SCALARS:
    return _SCALARS[base]
  raise RecAttendError('include/recattend.h: %s: no ctypes mapping for the type "%s"' % (name, ' '.join(words)))


def _struct_members(text, name):
  """[(member, ctypes type)] of `typedef struct name { ... } name;` whose members are ints and long longs; [] when the text
  has no such struct."""
  struct = re.search(r'typedef\s+struct\s+%s\s*\{([^{}]*)\}\s*%s\s*;' % (name, name), text)
  out = []
  for decl in filter(None, (d.strip() for d in struct.group(1).split(';'))) if struct else ():
    m = re.match(r'(long\s+long|int)\s+(\w+(?:\s*,\s*\w+)*)$', decl)
    if m is None:
      raise RecAttendError('include/recattend.h: %s: member "%s" is neither an int nor a long long' % (name, decl))
    out += [(n, _MEMBERS[' '.join(m.group(1).split())]) for n in re.findall(r'\w+', m.group(2))]
  return out


def read_header(text, geo_fields=None):
  """(signatures, constants, ra_ctrl_desc field names) of the text of recattend.h.  signatures: {name: (restype,
  [argtypes])} of every `ret ra_name(args);`, constants: {name: int} of every `#define RA_NAME integer`.  The header is
  the only statement of the ABI, so a prototype this cannot split or a type it has no mapping for is an error, never a guess."""
  geo_fields = [] if geo_fields is None else geo_fields  # receives struct ra_image_geo's members, where the text has it
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  constants = {m.group(1): int(m.group(2))
               for m in re.finditer(r'^#define[ \t]+(RA_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', text, re.M)}
  text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
  struct = re.search(r'typedef\s+struct\s+ra_ctrl_desc\s*\{([^{}]*)\}\s*ra_ctrl_desc\s*;', text)
  if struct is None:
    raise RecAttendError('include/recattend.h: struct ra_ctrl_desc not found')
  fields = []
  for decl in filter(None, (d.strip() for d in struct.group(1).split(';'))):
    if not re.match(r'int\s+\w+(\s*,\s*\w+)*$', decl):
      raise RecAttendError('include/recattend.h: ra_ctrl_desc: member "%s" is not an int' % decl)
    fields += re.findall(r'\w+', decl)[1:]
  geo_fields.extend(_struct_members(text, 'ra_image_geo'))
  text = re.sub(r'(typedef\s+struct\s+\w+|enum)\s*\{[^{}]*\}\s*\w*\s*;', '', text)
  text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', text, flags=re.S)
  signatures = {}
  for stmt in filter(None, (s.strip() for s in text.split(';'))):
    m = re.match(r'([\w\s*]+?)\b(ra_\w+)\s*\(([^()]*)\)$', stmt)
    if m is None:
      raise RecAttendError('include/recattend.h: cannot split the prototype "%s"' % ' '.join(stmt.split()))
    ret, name, params = m.groups()
    ret = re.findall(r'\w+|\*', ret)
    res = C.c_char_p if ret == ['const', 'char', '*'] else _ctype(ret, name)
    args = []
    if params.split() != ['void']:
      for p in params.split(','):
        words = [w for w in re.findall(r'\w+|\*', p) if w != 'const']
        if len(words) < 2 or words[-1] == '*' or re.sub(r'[\w\s*]', '', p):
          raise RecAttendError('include/recattend.h: %s: cannot split the parameter "%s"' % (name, ' '.join(p.split())))
        args.append(_ctype(words[:-1], name))  # the last word is the parameter's name
    signatures[name] = (res, args)
  return signatures, constants, fields


# name -> (restype, argtypes) of every symbol, the RA_* integer constants and the controller descriptor, all as
# include/recattend.h states them
_geo_fields = []
with open(HEADER_PATH) as _f:
  SIGNATURES, CONSTANTS, _fields = read_header(_f.read(), _geo_fields)
CtrlDesc._fields_ = [(n, C.c_int) for n in _fields]
ImageGeo._fields_ = _geo_fields
globals().update(CONSTANTS)  # RA_ABI_VERSION, RA_E_*, RA_CONV_TRANSPOSED, RA_ATTN_STRIDE, RA_PASTE_*, RA_RESAMPLE_*

_lib = None


def lib():
  """The loaded library; raises RecAttendError if it (or any symbol) is missing."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise RecAttendError(
          'librecattend.so not found at %s — build it with `python -c "import '
          '__graft_entry__ as g; g.build()"` (no CPU fallback exists)' % LIB_PATH)
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
      try:
        fn = getattr(handle, name)
      except AttributeError:
        raise RecAttendError('librecattend.so lacks symbol %s' % name)
      fn.restype = res
      fn.argtypes = args
    if handle.ra_version() != RA_ABI_VERSION:
      raise RecAttendError('librecattend.so has ABI version %d, this binding was written against %d: rebuild it '
                           '(__graft_entry__.build())' % (handle.ra_version(), RA_ABI_VERSION))
    _lib = handle
  return _lib


def check(rc, what):
  """Turn a non-zero return code into an exception carrying ra_last_error_string()."""
  if rc != 0:
    msg = lib().ra_last_error_string()
    raise RecAttendError('%s failed with code %d: %s' % (what, rc, (msg or b'').decode()))


def ptr(t):
  """Raw data pointer of a torch tensor / numpy array / None."""
  if t is None:
    return None
  if isinstance(t, int):
    return t
  if hasattr(t, 'data_ptr'):
    return t.data_ptr()
  return t.ctypes.data


def stream_ptr():
  import torch
  return torch.cuda.current_stream().cuda_stream


class quiet_capture(object):
  """Context for a HIP-graph capture: Python's cyclic garbage collector is parked for its duration.  A
  collection that happens to run inside the capture can destroy an old graph, event or pinned buffer,
  and the runtime aborts the process on such a call while a stream is capturing (seen once the test
  suite ran decode pipelines before a training-step capture)."""

  def __enter__(self):
    import gc
    gc.collect()
    self._was = gc.isenabled()
    gc.disable()
    return self

  def __exit__(self, *exc):
    import gc
    if self._was:
      gc.enable()
    return False
