"""The render stage without a device: the oracle (tests/render_oracle.py) on cases derived by hand from the reference's lines,
the colour rule of the ground-truth image, the two channel conventions on the bytes of a decoded file, the colour PNG writer,
the count file's text and the new command-line flags."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import analysis
import ra_native as rn
import ra_ops as ops
import render_oracle as ro
from utils import png


# ---- the oracle by hand
def test_oracle_add_wraps_like_uint8():
  y = np.zeros((2, 1, 3), np.float32)
  y[0, 0, :2] = 1.0  # plane 0 on pixels 0, 1; plane 1 on pixels 1, 2: they overlap on pixel 1
  y[1, 0, 1:] = 1.0
  cols = [[192, 57, 43], [243, 156, 18]]  # rows 0 and 1 of the palette: 192 + 243 = 435 -> 435 - 256 = 179
  img = ro.add_image(y, cols)
  assert img[0].tolist() == [[192, 57, 43], [179, 213, 61], [243, 156, 18]]
  # a plane of value 2.0 doubles the colour, mod 256: 2 * 192 = 384 -> 128, 114, 86
  assert ro.add_image(np.full((1, 1, 1), 2.0, np.float32), cols[:1])[0, 0].tolist() == [128, 114, 86]
  # a soft 0.7 is truncated to 0 by the uint8 cast and draws nothing
  assert ro.add_image(np.full((1, 1, 1), 0.7, np.float32), cols[:1])[0, 0].tolist() == [0, 0, 0]
  # the batch form hands cv2.imwrite the swapped array
  assert ro.render_instances(y[None])[0, 0].tolist() == [[43, 57, 192], [61, 213, 179], [18, 156, 243]]


def test_oracle_first_decides_per_channel():
  y = np.ones((2, 1, 2), np.float32)
  y[1, 0, 0] = 0.0  # the later plane covers pixel 1 only
  cols = [[255, 0, 17], [9, 200, 255]]  # the earlier colour leaves channel 1 at zero
  img = ro.first_image(y, cols)
  # pixel 0: the earlier colour alone; pixel 1: the later plane fills exactly the channel the earlier one left at 0
  assert img[0].tolist() == [[255, 0, 17], [255, 200, 17]]
  # an earlier EMPTY pixel takes the later colour whole
  y2 = np.array([[[0.0]], [[1.0]]], np.float32)
  assert ro.first_image(y2, cols)[0, 0].tolist() == [9, 200, 255]


# ---- the colour rule of the ground-truth image (analysis.py:168-182)
def test_groundtruth_colours_by_hand():
  cmap = np.array(analysis.INSTANCE_CMAP)
  # two planes claim output 1: the first gets its colour, the second the last colour of the palette; the third matches output 0
  iou = np.zeros((1, 3, 3))
  iou[0, 1, 0], iou[0, 1, 1], iou[0, 0, 2] = 0.9, 0.4, 0.5
  got = analysis.groundtruth_colours(iou)
  assert got.dtype == np.uint8 and got.shape == (1, 3, 3)
  assert got[0].tolist() == [cmap[1].tolist(), cmap[21].tolist(), cmap[0].tolist()]
  # an empty plane in the middle: its column is all zero, arg-max 0, and it CONSUMES colour 0; the next plane that matches
  # output 0 then falls back to the end of the palette
  iou = np.zeros((1, 2, 3))
  iou[0, 1, 0], iou[0, 0, 2] = 0.7, 0.6
  assert analysis.groundtruth_colours(iou)[0].tolist() == [cmap[1].tolist(), cmap[0].tolist(), cmap[21].tolist()]
  # 24 planes all matching output 0: colour 0, then 21, 20, .., 1, and with all 22 used the previous colour stays
  got = analysis.groundtruth_colours(np.zeros((1, 3, 24)))
  assert got[0].tolist() == [cmap[i].tolist() for i in [0] + list(range(21, 0, -1)) + [1, 1]]
  # torch tensors are taken too, and the oracle says the same on random input
  rng = np.random.RandomState(3)
  iou = rng.rand(3, 7, 9) * (rng.rand(3, 7, 9) > 0.5)
  assert (analysis.groundtruth_colours(torch.from_numpy(iou)) == ro.groundtruth_colours(iou)).all()
  # a winning index beyond the palette raises, as flag[max_idx] does there
  iou = np.zeros((1, 23, 1))
  iou[0, 22, 0] = 1.0
  with pytest.raises(IndexError):
    analysis.groundtruth_colours(iou)
  with pytest.raises(IndexError):
    ro.groundtruth_colours(iou)


def test_tables():
  assert len(analysis.INSTANCE_CMAP) == 22 and analysis.INSTANCE_CMAP[21] == (63, 29, 82)  # 319 stored as uint8
  assert (np.array(analysis.INSTANCE_CMAP) == ro.CMAP).all()
  assert len(analysis.ORIENTATION_WHEEL) == 8 and (np.array(analysis.ORIENTATION_WHEEL) == ro.WHEEL).all()
  assert analysis.ORIENTATION_WHEEL[0] == (255, 17, 0) and analysis.ORIENTATION_WHEEL[6] == (9, 0, 255)


def _file_rgb(path):
  """The R, G, B samples of an 8-bit RGB PNG written with filter 0, read with nothing but zlib: [H,W,3]."""
  data = open(path, 'rb').read()
  chunks = {tag: payload for tag, payload, _ in png.iter_chunks(data)}
  W, H = struct.unpack('>II', chunks[b'IHDR'][:8])
  rows = np.frombuffer(zlib.decompress(chunks[b'IDAT']), np.uint8).reshape(H, 3 * W + 1)
  return rows[:, 1:].reshape(H, W, 3)


def test_channel_conventions_on_the_bytes_of_a_file(tmp_path):
  # an instance image: what the reference hands cv2.imwrite is swapped, so the file's R, G, B is the cmap row
  y = np.zeros((1, 2, 1, 2), np.float32)
  y[0, 0, 0, 0] = y[0, 1, 0, 1] = 1.0
  a = png.write_colour8(str(tmp_path / 'ins.png'), ro.render_instances(y)[0])
  assert _file_rgb(a)[0].tolist() == [list(analysis.INSTANCE_CMAP[0]), list(analysis.INSTANCE_CMAP[1])]
  # an orientation image goes to cv2.imwrite unswapped: the file's R, G, B is the wheel row REVERSED
  d = np.zeros((1, 1, 2, 8))
  d[0, 0, 0, 0] = d[0, 0, 1, 4] = 1.0
  b = png.write_colour8(str(tmp_path / 'ori.png'), ro.orientation_image(d, np.ones((1, 1, 2)))[0])
  assert _file_rgb(b)[0].tolist() == [list(analysis.ORIENTATION_WHEEL[0])[::-1], list(analysis.ORIENTATION_WHEEL[4])[::-1]]
  assert _file_rgb(b)[0].tolist() == [[0, 17, 255], [213, 255, 0]]
  # the mask: 0 blanks the pixel
  assert ro.orientation_image(d, np.array([[[1.0, 0.0]]]))[0, 0].tolist() == [[255, 17, 0], [0, 0, 0]]


# ---- utils/png: the colour writer
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (64, 67)])
def test_colour_png_round_trip(tmp_path, shape):
  H, W = shape
  img = np.random.RandomState(H * W).randint(0, 256, (H, W, 3)).astype(np.uint8)
  path = str(tmp_path / 'a.png')
  assert png.write_colour8(path, img) == path
  assert (png.read_colour8(path) == img).all()
  data = open(path, 'rb').read()
  assert data == png.encode_colour8(img) and data[:8] == png.SIGNATURE
  tags = [tag for tag, _, _ in png.iter_chunks(data)]
  assert tags == [b'IHDR', b'IDAT', b'IEND']
  ihdr = next(p for t, p, _ in png.iter_chunks(data) if t == b'IHDR')
  assert struct.unpack('>IIBBBBB', ihdr) == (W, H, 8, 2, 0, 0, 0)  # 8-bit, colour type 2 (RGB), no interlace
  assert (_file_rgb(path) == img[:, :, ::-1]).all()  # R, G, B in the file
  assert len(png.encode_colour8(img, level=0)) > H * W * 3  # stored, not deflated
  # a view with strides is written as its values
  assert (png.decode_colour8(png.encode_colour8(img[:, ::-1])) == img[:, ::-1]).all()


def test_colour_png_hand_built_file_and_refusals():
  # R, G, B = (1, 2, 3), (4, 5, 6) by hand -> cv2's B, G, R
  raw = bytes([0, 1, 2, 3, 4, 5, 6])
  chunk = lambda tag, d: struct.pack('>I', len(d)) + tag + d + struct.pack('>I', zlib.crc32(tag + d) & 0xffffffff)
  data = png.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', 2, 1, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw)) + \
      chunk(b'IEND', b'')
  assert png.decode_colour8(data).tolist() == [[[3, 2, 1], [6, 5, 4]]]
  assert png.encode_colour8(np.array([[[3, 2, 1], [6, 5, 4]]], np.uint8), level=6) == data
  for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), np.float32),
              np.zeros((0, 2, 3), np.uint8)):
    with pytest.raises(ValueError):
      png.encode_colour8(bad)


# ---- CountAnalyzer
def test_count_file_text(tmp_path, monkeypatch):
  y = np.zeros((2, 3, 4, 4), np.float32)
  y[0, 0, 1, 1] = y[0, 2, 0, 0] = y[1, 1, 3, 3] = 1.0
  s_gt = np.array([[1, 1, 1], [1, 0, 0]], np.float32)
  # f_count_out runs a kernel; its definition (:766-770) is a plane that has a pixel
  monkeypatch.setattr(analysis, 'f_count_out', lambda t: (t.flatten(2).sum(2) > 0).to(torch.float32))
  path = str(tmp_path / 'count.csv')
  c = analysis.CountAnalyzer(path)
  assert open(path).read() == 'Image ID,Count Out,Count GT\n'
  c.stage({'y_out': torch.from_numpy(y), 's_gt': torch.from_numpy(s_gt), 'indices': [7, 8]})
  c.finalize()
  assert open(path).read() == 'Image ID,Count Out,Count GT\n7,2,3\n8,1,1\n' == ro.count_text([7, 8], y, s_gt)
  c.stage({'y_out': torch.from_numpy(y[:1]), 's_gt': torch.from_numpy(s_gt[:1]), 'indices': [9]})  # appended, as there
  assert open(path).read().endswith('8,1,1\n9,2,3\n')


# ---- the command lines
def test_new_flags_are_off_by_default_and_old_refusals_stand(tmp_path):
  import cityscapes_eval
  import cmd_args_parser as cap
  import fg_model_eval
  import full_model_eval
  a = full_model_eval.build_parser().parse_args([])
  assert a.render is False and a.render_gt_instances is False
  a = full_model_eval.build_parser().parse_args(['--render', '--render_gt_instances'])
  assert a.render and a.render_gt_instances
  c = cityscapes_eval.build_parser().parse_args([])
  assert c.render_instances is False and c.render_gt is False
  assert cityscapes_eval.build_parser().parse_args(['--render_instances']).render_instances
  f = fg_model_eval.build_parser().parse_args([])
  assert f.render_orientation is False and f.render_ori is False
  f = fg_model_eval.build_parser().parse_args(['--render_orientation'])
  assert f.render_orientation and not f.render_ori
  # none of them is a reference flag: the tables that restate the reference's parsers do not list them
  for table in (cap.EVAL_FLAGS, cap.DATA_FLAGS, cap.CITYSCAPES_EVAL_FLAGS, cap.FG_EVAL_FLAGS):
    assert not {'render', 'render_gt_instances', 'render_instances', 'render_orientation'} & {n for n, _, _ in table}
  for parser in (full_model_eval, cityscapes_eval, fg_model_eval):
    text = parser.build_parser().format_help()
    assert text.count('not a reference flag') >= 1
  # the reference's flags are refused as before, and now say where the image is built
  with pytest.raises(rn.RecAttendError, match='orientation') as e:
    fg_model_eval.make_opt(fg_model_eval.build_parser().parse_args(['--render_ori']))
  assert '--render_orientation' in str(e.value)
  with pytest.raises(rn.RecAttendError, match='ground truth') as e:
    cityscapes_eval.make_opt(cityscapes_eval.build_parser().parse_args(['--render_gt']))
  assert '--render_instances' in str(e.value)
  assert fg_model_eval.make_opt(fg_model_eval.build_parser().parse_args(['--render_orientation']))['render_ori'] is False


def test_render_without_labels_names_what_is_missing(tmp_path):
  import full_model_eval
  for flag in ('--render', '--render_gt_instances'):
    with pytest.raises(rn.RecAttendError, match='y_gt') as e:  # synthetic input has no labels
      full_model_eval.main(['--model_id', 'm', '--results', str(tmp_path), flag])
    assert flag in str(e.value) and 's_gt' in str(e.value)
  inp = str(tmp_path / 'in.npz')
  np.savez(inp, x=np.zeros((1, 8, 8, 3), np.float32), y_gt=np.zeros((1, 2, 8, 8), np.float32))
  with pytest.raises(rn.RecAttendError, match='lacks s_gt') as e:
    full_model_eval.main(['--model_id', 'm', '--results', str(tmp_path), '--input', inp, '--render'])
  assert '--render' in str(e.value) and 'lacks y_gt' not in str(e.value)
  np.savez(inp, x=np.zeros((1, 8, 8, 3), np.float32))
  with pytest.raises(rn.RecAttendError, match='lacks y_gt and s_gt'):
    full_model_eval.main(['--model_id', 'm', '--results', str(tmp_path), '--input', inp, '--render', '--render_gt_instances'])


def test_wrappers_refuse_cpu_tensors(tmp_path):
  y = torch.zeros(1, 2, 4, 4)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.render_instances(y)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.render_instances(y, first=True)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.render_orientation(torch.zeros(1, 2, 2, 8), torch.zeros(1, 4, 4))
  with pytest.raises(rn.RecAttendError):
    analysis.RenderInstanceAnalyzer(str(tmp_path / 'out'), ['a']).stage({'y_out': y, 'indices': [0]})


def test_entry_points_check_their_arguments_without_a_device():
  lib = rn.lib()
  assert (rn.RA_RENDER_ADD, rn.RA_RENDER_FIRST) == (0, 1) and rn.RA_RENDER_MAX_T >= 32
  p = 4096  # never dereferenced: every call below is refused before a launch
  assert lib.ra_render_instances_u8(None, 1, 1, 4, 4, p, 0, p, None) == rn.RA_E_INVALID
  assert lib.ra_render_instances_u8(p, 1, 1, 4, 4, p, 2, p, None) == rn.RA_E_INVALID and b'mode' in lib.ra_last_error_string()
  assert lib.ra_render_instances_u8(p, 1, 0, 4, 4, p, 0, p, None) == rn.RA_E_SHAPE
  assert lib.ra_render_instances_u8(p, 1, rn.RA_RENDER_MAX_T + 1, 4, 4, p, 1, p, None) == rn.RA_E_SHAPE
  assert lib.ra_render_instances_u8(p, 1, 1, 1 << 16, 1 << 15, p, 0, p, None) == rn.RA_E_SHAPE
  assert b'ra_render_instances_u8' in lib.ra_last_error_string()
  assert lib.ra_render_orientation_u8(p, 1, 4, 4, 8, None, 8, 8, p, p, None) == rn.RA_E_INVALID
  for C in (1, 17):
    assert lib.ra_render_orientation_u8(p, 1, 4, 4, C, p, 8, 8, p, p, None) == rn.RA_E_SHAPE
  assert lib.ra_render_orientation_u8(p, 1, 4, 0, 8, p, 8, 8, p, p, None) == rn.RA_E_SHAPE
  assert b'ra_render_orientation_u8' in lib.ra_last_error_string()
