"""8-bit greyscale PNG files on zlib + struct only (what cv2.imwrite(name, uint8 [H,W]) produces for the instance
masks of analysis.py:255-257; cv2 is not part of this stack).  One IHDR, one IDAT, one IEND chunk; filter type 0 on
every row.  `decode_gray8` reads exactly that subset back (tests, tools).

`decode_gray16` / `read_gray16` read 16-bit greyscale files (*_gtFine_instanceIds.png of the Cityscapes ground truth) as
other encoders write them: any number of IDAT chunks and all five row filters of the PNG specification (section 9).  A
file whose rows use None, Sub and Up is undone a row at a time (tens of ms for 1024 x 2048); one that holds Average or Paeth
rows is undone by the library's compiled loop (ra_png_unfilter_u8, host code), and by anti-diagonals in NumPy, about a
second for that size, where librecattend.so cannot be loaded: this module imports and works without it.

`decode_colour8` / `read_colour8` read what cv2.imread(path) reads for the datasets' colour files (leftImg8bit, KITTI's and
CVPPP's images and colour label files): uint8 [H,W,3] in cv2's BGR order from 8-bit RGB, RGBA (alpha dropped), palette
(depths 1, 2, 4, 8) and grey files.  Interlaced files and 16-bit colour are refused.

`encode_colour8` / `write_colour8` write such a BGR array as an 8-bit RGB file (what cv2.imwrite stores for the colour images
of analysis.py's render analyzers), with the same one-IDAT, filter-0 layout as `encode_gray8`.

`encode_gray8_dev` / `encode_colour8_dev` / `write_gray8_dev` / `write_colour8_dev` take a BATCH of images in device memory
and return / write one file per image: the deflate stage runs on the device (ra_ops.png_deflate, csrc/ra_png.hip — filter 0, a
fixed-Huffman run code within each row), only the finished streams leave it, and `wrap` puts the container around a stream.
The files decode to the same pixels as the host writers' files; their bytes differ and they are 2.5 x (flat colour) to 7 x (binary masks) as large as zlib
level 6 makes them, so the output stages use them only when asked (device_png).  code='dynamic' selects the encoder's second
stream format, one dynamic-Huffman block per image with a code built on the device: a mask then takes about a fifth of the fixed
format's bytes, 1.15 - 1.25 x zlib level 6 (profiles/png_dynamic.txt).  Only these four need the library and a GPU."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(tag, data):
  return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def encode_gray8(img, level=6):
  """img: uint8 [H,W] -> the bytes of a PNG file (colour type 0, bit depth 8, no interlace)."""
  img = np.ascontiguousarray(img)
  if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
    raise ValueError('encode_gray8 needs a uint8 [H,W] array, got %s %s' % (img.dtype, img.shape))
  H, W = img.shape
  rows = np.zeros((H, W + 1), dtype=np.uint8)  # a filter-type byte (0 = None) in front of every row
  rows[:, 1:] = img
  ihdr = struct.pack('>IIBBBBB', W, H, 8, 0, 0, 0, 0)
  return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_gray8(path, img, level=6):
  with open(path, 'wb') as f:
    f.write(encode_gray8(img, level))


def iter_chunks(data):
  """(tag, payload, stored crc) of every chunk; raises ValueError on a bad signature or a truncated file."""
  if data[:8] != SIGNATURE:
    raise ValueError('not a PNG file')
  pos = 8
  while pos < len(data):
    if pos + 8 > len(data):
      raise ValueError('truncated PNG chunk header')
    n, = struct.unpack('>I', data[pos:pos + 4])
    tag = data[pos + 4:pos + 8]
    if pos + 12 + n > len(data):
      raise ValueError('truncated PNG chunk')
    crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
    yield tag, data[pos + 8:pos + 8 + n], crc
    pos += 12 + n


def decode_gray8(data):
  """The inverse of encode_gray8 (8-bit greyscale, filter 0 only, CRCs checked) -> uint8 [H,W]."""
  shape, idat = None, b''
  for tag, payload, crc in iter_chunks(data):
    if zlib.crc32(tag + payload) & 0xffffffff != crc:
      raise ValueError('bad CRC in chunk %r' % tag)
    if tag == b'IHDR':
      W, H, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', payload)
      if (depth, colour, comp, flt, lace) != (8, 0, 0, 0, 0):
        raise ValueError('only 8-bit greyscale, non-interlaced PNG files are read here')
      shape = (H, W)
    elif tag == b'IDAT':
      idat += payload
  if shape is None:
    raise ValueError('no IHDR chunk')
  rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(shape[0], shape[1] + 1)
  if rows[:, 0].any():
    raise ValueError('only filter type 0 is read here')
  return rows[:, 1:].copy()


def read_gray8(path):
  with open(path, 'rb') as f:
    return decode_gray8(f.read())


def _unfilter_rows(raw, H, stride, bpp):
  """_unfilter for files whose rows use the filters None, Sub and Up only: one NumPy expression per row."""
  out = np.zeros((H, stride), dtype=np.uint8)
  prev = np.zeros(stride, dtype=np.int64)
  for r in range(H):
    ft, v = raw[r, 0], raw[r, 1:].astype(np.int64)
    if ft == 2:  # Up
      v = (v + prev) & 255
    elif ft == 1:  # Sub: a running sum (mod 256) along each of the bpp byte lanes
      for k in range(bpp):
        v[k::bpp] = np.cumsum(v[k::bpp]) & 255
    out[r] = prev = v
  return out


def _unfilter_diagonals(raw, H, stride, bpp):
  """_unfilter for files that hold Average or Paeth rows.  A byte of those needs the reconstructed bytes to its left, above
  it and above left, so neither a row nor a column can be undone at once; the pixels of one anti-diagonal (row + column
  constant) need only the two diagonals before them.  Walk the H + W - 1 diagonals, every one a NumPy expression over its
  pixels with the predictor chosen by the row's filter type: a 1024 x 2048 16-bit image takes 3071 steps, not 4 M."""
  W = stride // bpp
  ft = raw[:, 0].astype(np.int64)[:, None]
  x = raw[:, 1:].astype(np.int64).reshape(H, W, bpp)
  out = np.zeros((H + 1, W + 1, bpp), dtype=np.int64)  # a zero row above and a zero column to the left (9.2)
  for d in range(H + W - 1):
    r = np.arange(max(0, d - W + 1), min(H - 1, d) + 1)
    c = d - r
    a, b, cc = out[r + 1, c], out[r, c + 1], out[r, c]  # left, above, above left
    pa, pb, pc = np.abs(b - cc), np.abs(a - cc), np.abs(a + b - 2 * cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    f = ft[r]
    pred = np.where(f == 0, 0, np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, paeth))))
    out[r + 1, c + 1] = (x[r, c] + pred) & 255
  return out[1:, 1:].reshape(H, stride).astype(np.uint8)


def _unfilter(raw, H, stride, bpp):
  """The scanlines of a non-interlaced image with the filter of every row undone (PNG specification, 9.2): raw holds H rows
  of one filter-type byte + stride bytes, bpp = bytes per complete pixel.  -> uint8 [H, stride]."""
  if len(raw) != H * (stride + 1):
    raise ValueError('PNG image data has %d bytes, %d expected' % (len(raw), H * (stride + 1)))
  raw = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride + 1)
  if raw[:, 0].max() > 4:
    r = int(np.argmax(raw[:, 0] > 4))
    raise ValueError('PNG row %d has filter type %d' % (r, raw[r, 0]))
  if not (raw[:, 0] >= 3).any():
    return _unfilter_rows(raw, H, stride, bpp)
  return (_unfilter_native if _native() else _unfilter_diagonals)(raw, H, stride, bpp)


_NATIVE = []  # [the loaded library, or None where it cannot be loaded], filled at the first file that needs it


def _native():
  if not _NATIVE:
    try:
      import ra_native
      _NATIVE.append(ra_native.lib())
    except (ImportError, OSError, RuntimeError):
      _NATIVE.append(None)
  return _NATIVE[0]


def _unfilter_native(raw, H, stride, bpp):
  """_unfilter_diagonals' result from ra_png_unfilter_u8: one compiled pass over the scanlines."""
  raw = np.ascontiguousarray(raw)
  out = np.empty((H, stride), dtype=np.uint8)
  if _native().ra_png_unfilter_u8(raw.ctypes.data, H, stride, bpp, out.ctypes.data) != 0:
    raise ValueError((_native().ra_last_error_string() or b'ra_png_unfilter_u8 failed').decode())
  return out


def decode_gray16(data):
  """16-bit greyscale, non-interlaced PNG (colour type 0, bit depth 16; all five row filters; CRCs checked) -> uint16 [H,W]."""
  shape, idat = None, b''
  for tag, payload, crc in iter_chunks(data):
    if zlib.crc32(tag + payload) & 0xffffffff != crc:
      raise ValueError('bad CRC in chunk %r' % tag)
    if tag == b'IHDR':
      W, H, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', payload)
      if (depth, colour, comp, flt, lace) != (16, 0, 0, 0, 0):
        raise ValueError('only 16-bit greyscale, non-interlaced PNG files are read here (bit depth %d, colour type %d, '
                         'interlace %d)' % (depth, colour, lace))
      shape = (H, W)
    elif tag == b'IDAT':
      idat += payload
  if shape is None:
    raise ValueError('no IHDR chunk')
  H, W = shape
  try:
    raw = zlib.decompress(idat)
  except zlib.error as e:
    raise ValueError('PNG image data does not inflate: %s' % e)
  rows = _unfilter(raw, H, 2 * W, 2)
  return (rows[:, 0::2].astype(np.uint16) << 8) | rows[:, 1::2]  # big-endian samples


def read_gray16(path):
  with open(path, 'rb') as f:
    return decode_gray16(f.read())


_CHANNELS = {0: 1, 2: 3, 3: 1, 6: 4}  # samples per pixel of the colour types read by decode_colour8


def decode_colour8(data):
  """What cv2.imread(path) (IMREAD_COLOR) gives for an 8-bit PNG: uint8 [H,W,3] in BGR order.  Colour type 2 (RGB) and 6
  (RGBA: the alpha channel is dropped, not blended) at bit depth 8, 3 (palette) at depths 1, 2, 4, 8 expanded through PLTE
  (tRNS ignored), 0 (grey) at depth 8 replicated to three channels; any number of IDAT chunks, all five row filters, CRCs
  checked.  Interlaced files, 16-bit samples and everything else raise ValueError."""
  head, idat, palette = None, b'', None
  for tag, payload, crc in iter_chunks(data):
    if zlib.crc32(tag + payload) & 0xffffffff != crc:
      raise ValueError('bad CRC in chunk %r' % tag)
    if tag == b'IHDR':
      if len(payload) != 13:
        raise ValueError('IHDR chunk of %d bytes' % len(payload))
      W, H, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', payload)
      ok = (depth == 8 and colour in (0, 2, 6)) or (colour == 3 and depth in (1, 2, 4, 8))
      if not ok or (comp, flt, lace) != (0, 0, 0) or W < 1 or H < 1:
        raise ValueError('only 8-bit RGB, RGBA and grey and 1-, 2-, 4-, 8-bit palette PNG files without interlace are read here '
                         '(%d x %d, bit depth %d, colour type %d, interlace %d)' % (W, H, depth, colour, lace))
      head = (H, W, depth, colour)
    elif tag == b'PLTE':
      if len(payload) % 3 or not payload:
        raise ValueError('PLTE chunk of %d bytes' % len(payload))
      palette = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3)
    elif tag == b'IDAT':
      idat += payload
  if head is None:
    raise ValueError('no IHDR chunk')
  H, W, depth, colour = head
  try:
    raw = zlib.decompress(idat)
  except zlib.error as e:
    raise ValueError('PNG image data does not inflate: %s' % e)
  ch = _CHANNELS[colour]
  stride = (W * ch * depth + 7) // 8
  rows = _unfilter(raw, H, stride, max(1, ch * depth // 8))
  if colour == 3:
    if palette is None:
      raise ValueError('a palette PNG file without a PLTE chunk')
    if depth < 8:  # the leftmost sample in the high bits; the padding bits of a row are dropped
      bits = np.unpackbits(rows, axis=1).reshape(H, -1, depth)[:, :W]
      rows = (bits << np.arange(depth - 1, -1, -1, dtype=np.uint8)).sum(axis=2).astype(np.uint8)
    if int(rows.max()) >= len(palette):
      raise ValueError('palette index %d, the palette has %d entries' % (int(rows.max()), len(palette)))
    rgb = palette[rows]
  elif colour == 0:
    rgb = np.repeat(rows[:, :, None], 3, axis=2)
  else:
    rgb = rows.reshape(H, W, ch)[:, :, :3]
  return np.ascontiguousarray(rgb[:, :, ::-1])


def read_colour8(path):
  with open(path, 'rb') as f:
    return decode_colour8(f.read())


def encode_colour8(img, level=6):
  """What cv2.imwrite(name, img) stores for a uint8 [H,W,3] array in cv2's BGR order: the bytes of an 8-bit RGB PNG file
  (colour type 2, bit depth 8, no interlace; one IHDR, one IDAT, one IEND chunk, filter type 0 on every row).
  decode_colour8(encode_colour8(img)) is img."""
  img = np.asarray(img)
  if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
    raise ValueError('encode_colour8 needs a uint8 [H,W,3] array, got %s %s' % (img.dtype, img.shape))
  H, W, _ = img.shape
  rows = np.zeros((H, 3 * W + 1), dtype=np.uint8)  # a filter-type byte (0 = None) in front of every row
  rows[:, 1:] = img[:, :, ::-1].reshape(H, 3 * W)  # B, G, R in memory -> R, G, B in the file
  ihdr = struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)
  return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_colour8(path, img, level=6):
  with open(path, 'wb') as f:
    f.write(encode_colour8(img, level))
  return path


def wrap(H, W, colour_type, zstream):
  """The bytes of a PNG file around a finished zlib stream of its scanlines: signature, IHDR (bit depth 8, no interlace;
  colour_type 0 = grey, 2 = RGB), one IDAT whose CRC-32 is taken here over the compressed bytes, IEND."""
  if colour_type not in (0, 2) or H < 1 or W < 1:
    raise ValueError('wrap: %d x %d, colour type %d (0 = grey or 2 = RGB, at least one pixel)' % (H, W, colour_type))
  ihdr = struct.pack('>IIBBBBB', W, H, 8, colour_type, 0, 0, 0)
  return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', bytes(zstream)) + _chunk(b'IEND', b'')


def encode_gray8_dev(t, plane_index=None, code='fixed'):
  """t: a DEVICE tensor, uint8 [N,H,W] or float32 [M,H,W] (written as (t * 255).to(uint8), 0 <= t <= 1; plane_index then picks
  the planes to write, in its order) -> the bytes of one PNG file per image, a list.  The deflate stage runs on the device
  (ra_ops.png_deflate: filter 0, a run code within each row); the files decode to the pixels encode_gray8 stores, their
  bytes differ.  code: the stream format, 'fixed' or 'dynamic' (ra_ops.png_deflate).  Needs librecattend.so and a GPU."""
  import ra_ops
  if t.dim() != 3:
    raise ValueError('encode_gray8_dev needs a uint8 or float32 [N,H,W] tensor, got %s' % (tuple(t.shape),))
  H, W = int(t.shape[1]), int(t.shape[2])
  return [wrap(H, W, 0, z) for z in ra_ops.png_deflate(t.contiguous(), plane_index, code=code)]


def encode_colour8_dev(t, code='fixed'):
  """t: a DEVICE tensor uint8 [N,H,W,3] in cv2's B, G, R order -> the bytes of one 8-bit RGB PNG file per image, a list; the
  device twin of encode_colour8 (see encode_gray8_dev)."""
  import ra_ops
  if t.dim() != 4 or t.shape[3] != 3:
    raise ValueError('encode_colour8_dev needs a uint8 [N,H,W,3] tensor, got %s' % (tuple(t.shape),))
  H, W = int(t.shape[1]), int(t.shape[2])
  return [wrap(H, W, 2, z) for z in ra_ops.png_deflate(t.contiguous(), code=code)]


def _write_files(paths, files):
  paths = list(paths)
  if len(paths) != len(files):
    raise ValueError('%d paths for %d images' % (len(paths), len(files)))
  for path, data in zip(paths, files):
    with open(path, 'wb') as f:
      f.write(data)
  return paths


def write_gray8_dev(paths, t, plane_index=None, code='fixed'):
  """One file per image of encode_gray8_dev(t, plane_index, code), in the order of paths."""
  return _write_files(paths, encode_gray8_dev(t, plane_index, code))


def write_colour8_dev(paths, t, code='fixed'):
  """One file per image of encode_colour8_dev(t, code), in the order of paths."""
  return _write_files(paths, encode_colour8_dev(t, code))


def _wrap_ragged(streams, geo, colour_type):
  """One file per stream of a ragged call: stream k * B + b is wrapped with image b's own h, w."""
  sizes = [(int(h), int(w)) for _, h, w in np.asarray(geo).tolist()]
  return [wrap(sizes[i % len(sizes)][0], sizes[i % len(sizes)][1], colour_type, z) for i, z in enumerate(streams)]


def encode_gray8_ragged_dev(flat, geo, plane_index=None, code='fixed'):
  """encode_gray8_dev for a batch of MIXED sizes in one launch chain (ra_ops.png_deflate_ragged): flat is a DEVICE tensor of M
  planes, uint8 or float32 [M,P] ([P]: one plane), all laid out by the geometry geo [B,3] of (offset, h, w) -> the bytes of
  Np * B PNG files, file k * B + b = image b of plane plane_index[k] (None: plane k).  Every file holds the bytes
  encode_gray8_dev gives for that image alone."""
  import ra_ops
  if flat.dim() not in (1, 2):
    raise ValueError('encode_gray8_ragged_dev needs a uint8 or float32 [M,P] or [P] tensor, got %s' % (tuple(flat.shape),))
  return _wrap_ragged(ra_ops.png_deflate_ragged(flat.contiguous(), geo, plane_index, code=code), geo, 0)


def encode_colour8_ragged_dev(flat, geo, plane_index=None, code='fixed'):
  """encode_colour8_dev for a batch of MIXED sizes in one launch chain: flat is a DEVICE tensor uint8 [M,P,3] ([P,3]: one plane)
  in cv2's B, G, R order, what ra_ops.paint_instances(..., geo=...) writes (see encode_gray8_ragged_dev)."""
  import ra_ops
  if flat.dim() not in (2, 3) or flat.shape[-1] != 3:
    raise ValueError('encode_colour8_ragged_dev needs a uint8 [M,P,3] or [P,3] tensor, got %s' % (tuple(flat.shape),))
  return _wrap_ragged(ra_ops.png_deflate_ragged(flat.contiguous(), geo, plane_index, code=code), geo, 2)


def write_gray8_ragged_dev(paths, flat, geo, plane_index=None, code='fixed'):
  """One file per image of encode_gray8_ragged_dev(flat, geo, plane_index, code); paths in stream order (plane-major)."""
  return _write_files(paths, encode_gray8_ragged_dev(flat, geo, plane_index, code))


def write_colour8_ragged_dev(paths, flat, geo, plane_index=None, code='fixed'):
  """One file per image of encode_colour8_ragged_dev(flat, geo, plane_index, code); paths in stream order (plane-major)."""
  return _write_files(paths, encode_colour8_ragged_dev(flat, geo, plane_index, code))
