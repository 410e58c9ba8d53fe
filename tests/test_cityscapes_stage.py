"""The Cityscapes output stage without a GPU: the float64 oracle (tests/cs_oracle.py) pinned on cases computed by hand, the
PNG writer, the text-file line, the command line's defaults and refusals, and the loud failure without a device."""
import struct
import zlib

import numpy as np
import pytest

import cs_oracle as co
import ra_native as rn


# ---- the oracle, by hand
def test_resize_2x2_to_4x4_by_hand():
  a = np.array([[0.0, 1.0], [2.0, 3.0]])
  # source coordinate (d + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> clamped, 0.25, 0.75, clamped
  ax = np.array([0.0, 0.25, 0.75, 1.0])
  want = 2 * ax[:, None] + ax[None, :]
  assert np.allclose(co.resize_linear(a, 4, 4), want, atol=1e-15)
  i0, i1, w = co.taps(2, 4)
  assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and np.allclose(w, [0, 0.25, 0.75, 0])
  assert np.array_equal(co.resize_linear(a, 2, 2), a)  # equal size: the identity


def _blocks(Hs, Ws, C, chan_of_quadrant):
  sem = np.zeros((1, Hs, Ws, C), np.float32)
  h, w = Hs // 2, Ws // 2
  for q, c in enumerate(chan_of_quadrant):
    sem[0, (q // 2) * h:(q // 2 + 1) * h, (q % 2) * w:(q % 2 + 1) * w, c] = 1.0
  return sem


def test_instance_inside_a_car_region_is_a_car():
  sem = _blocks(8, 8, 9, [0, 3, 1, 5])       # top-right quadrant: channel 3 = car
  y = np.zeros((1, 2, 16, 16))
  y[0, 0, 1:6, 10:15] = 1.0                  # wholly inside the top-right quadrant, away from its borders
  y[0, 1, 10:15, 1:6] = 1.0                  # bottom-left: channel 1 = person
  v = co.vote(y, co.sem_full(sem, 16, 16))
  assert v.shape == (1, 2, 9)
  assert np.isclose(v[0, 0, 3], 25 / 256.0) and np.isclose(v[0, 0].sum(), 25 / 256.0)
  idx, lab = co.pick(v, np.array([[0.9, 0.8]]))
  assert idx.tolist() == [[2, 0]] and lab.tolist() == [[26, 24]]
  assert dict(co.LABELS)['car'] == 26 and [l for _, l in co.LABELS] == [24, 25, 26, 27, 28, 31, 32, 33]


def test_tie_takes_the_first_class_and_half_confidence_is_not_written():
  v = np.zeros((1, 3, 9))
  v[0, :, 2] = 0.125
  v[0, :, 6] = 0.125
  idx, lab = co.pick(v, np.array([[0.9, 0.5, 0.50001]]))
  assert idx.tolist() == [[1, -1, 1]] and lab.tolist() == [[25, -1, 25]]
  v[0, 0, 0] = 0.71                          # the background gate (vote[0] <= 0.7)
  v[0, 2, 0] = 0.7
  idx, _ = co.pick(v, np.array([[0.9, 0.9, 0.9]]))
  assert idx.tolist() == [[-1, 1, 1]]
  assert co.top2_gap(v)[0, 0] == 0.0
  idx, lab = co.pick(np.zeros((1, 1, 9)), np.array([[1.0]]))  # an all-zero instance with conf: the first class, as numpy.argmax
  assert idx.tolist() == [[0]] and lab.tolist() == [[24]]


def test_foreground_rules_one_channel_and_nine():
  s1 = np.array([0.2, 0.3, 0.31, 0.9]).reshape(1, 1, 4, 1)
  assert co.foreground(s1).ravel().tolist() == [0, 0, 1, 1]                # > 0.3
  s9 = np.zeros((1, 1, 4, 9))
  s9[0, 0, :, 0] = [0.2, 0.7, 0.71, 0.9]
  assert co.foreground(s9).ravel().tolist() == [1, 1, 0, 0]                # background <= 1 - 0.3


def test_remove_tiny_at_one_threshold_zeroes_conf_for_the_next():
  # on a one-label map given by hand: instance 0 is 0.9 on 30 pixels; instance 1 is 0.05 on 20 pixels and 0.9 on 4 -> 24
  # pixels at threshold 0.0 (> 10), 4 at 0.1 (tiny: removed), and at 0.0 AGAIN it is not written because conf was zeroed at 0.1
  y = np.zeros((1, 2, 8, 8))
  y[0, 0, :5, :6] = 0.9
  y[0, 1, 5:, :] = 0.05
  y[0, 1, 7, :4] = 0.9
  sem = np.zeros((1, 8, 8, 9), np.float32)
  sem[..., 4] = 1.0
  sem_h = co.sem_full(sem, 8, 8)
  p = co.threshold_chain(y, co.foreground(sem_h), sem_h, np.array([[1.0, 1.0]]), [0.0, 0.1, 0.0], remove_tiny=10)
  assert p[0]['conf'].tolist() == [[1.0, 1.0]] and p[0]['class_idx'].tolist() == [[3, 3]]
  assert p[1]['conf'].tolist() == [[1.0, 0.0]] and p[1]['y_out'][0, 1].sum() == 0 and p[1]['class_idx'].tolist() == [[3, -1]]
  assert p[2]['conf'].tolist() == [[1.0, 0.0]] and p[2]['class_idx'].tolist() == [[3, -1]]
  assert p[2]['sizes'][0, 1] > 10            # large enough again, and still not written: conf carried over
  assert p[0]['label_id'].tolist() == [[27, 27]]


# ---- the PNG writer
def test_png_round_trip_and_chunks():
  from utils import png
  rng = np.random.RandomState(3)
  for shape in ((1, 1), (5, 7), (64, 129)):
    img = rng.randint(0, 256, shape).astype(np.uint8)
    data = png.encode_gray8(img)
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    chunks = list(png.iter_chunks(data))
    assert [t for t, _, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    for tag, payload, crc in chunks:
      assert zlib.crc32(tag + payload) & 0xffffffff == crc
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (shape[1], shape[0], 8, 0, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == shape[0] * (shape[1] + 1)
    rows = np.frombuffer(raw, np.uint8).reshape(shape[0], shape[1] + 1)
    assert not rows[:, 0].any() and rows[:, 1:].tobytes() == img.tobytes()
    assert np.array_equal(png.decode_gray8(data), img)
  with pytest.raises(ValueError):
    png.encode_gray8(np.zeros((2, 2), np.float32))
  bad = bytearray(png.encode_gray8(np.zeros((2, 2), np.uint8)))
  bad[-5] ^= 1
  with pytest.raises(ValueError):
    png.decode_gray8(bytes(bad))


def test_png_file(tmp_path):
  from utils import png
  img = (np.arange(12).reshape(3, 4) * 20).astype(np.uint8)
  png.write_gray8(str(tmp_path / 'a.png'), img)
  assert np.array_equal(png.read_gray8(str(tmp_path / 'a.png')), img)


# ---- the text file
def test_text_line_format():
  import analysis
  assert analysis.cityscapes_line('munster_000051_000019_007.png', 26, 0.75) == 'munster_000051_000019_007.png 26 0.750000\n'
  assert analysis.CITYSCAPES_LABELS == co.LABELS
  assert analysis._stem('paris_000001_000019.png') == 'paris_000001_000019' and analysis._stem('x') == 'x'
  assert co.text_lines('frankfurt_1_2.png', np.zeros((3, 2, 2)), [0.9, 0.2, 0.8], [26, -1, 24], [2, -1, 0]) == [
      ('frankfurt_1_2_000.png', 26, 0.9), ('frankfurt_1_2_002.png', 24, 0.8)]


# ---- the command line
def test_cli_defaults_are_the_reference_s():
  import cityscapes_eval as ce
  a = ce.build_parser().parse_args([])
  # cityscapes_eval.py:260-272 and EvalArgsParser / DataArgsParser (cmd_args_parser.py:143-151,171-173)
  assert (a.threshold_list, a.analyzers, a.test, a.split_id, a.num_split, a.remove_tiny) == (None, None, False, -1, 100, 400)
  assert (a.foreground_folder, a.no_iou, a.render_gt, a.lrr_seg, a.output) == (None, False, False, False, None)
  assert (a.model_id, a.batch_size, a.results, a.split, a.dataset) == (None, 32, './results', 'valid', 'cvppp')
  opt = ce.make_opt(a)
  assert np.allclose(opt['threshold_list'], np.arange(10) * 0.1) and len(opt['threshold_list']) == 10
  assert opt['remove_tiny'] == 400 and opt['split'] == ['valid']
  ref_default = ['sbd', 'wt_cov', 'unwt_cov', 'fg_dice', 'fg_iou', 'fg_iou_all', 'bg_iou_all', 'avg_fp', 'avg_fn', 'avg_pr',
                 'avg_re', 'obj_pr', 'obj_re', 'count_acc', 'count_mse', 'dic', 'dic_abs']
  assert ce.DEFAULT_ANALYZERS == ref_default and opt['analyzers'] == [n for n in ref_default if not n.endswith('_all')]
  assert ce.make_opt(ce.build_parser().parse_args(['--test']))['analyzers'] == ['fg_iou']
  o = ce.make_opt(ce.build_parser().parse_args(['--threshold_list', '0.3,0.55', '--analyzers', 'sbd,dic', '--remove_tiny', '7']))
  assert o['threshold_list'] == [0.3, 0.55] and o['analyzers'] == ['sbd', 'dic'] and o['remove_tiny'] == 7
  assert ce.make_opt(ce.build_parser().parse_args(['--analyzers', '']))['analyzers'] == []
  assert ce.FG_THRESHOLD == co.FG_THRESHOLD == 0.3


@pytest.mark.parametrize('flag,word', [(['--lrr_seg'], 'LRR'), (['--foreground_folder', '/x'], 'foreground'),
                                       (['--render_gt'], 'ground truth')])
def test_cli_refuses_the_authors_file_readers(flag, word):
  import cityscapes_eval as ce
  with pytest.raises(rn.RecAttendError, match=word):
    ce.main(flag + ['--input', 'nowhere.npz', '--output', 'nowhere'])


def test_cli_needs_an_input():
  import cityscapes_eval as ce
  with pytest.raises(rn.RecAttendError, match='--input'):
    ce.main(['--output', 'nowhere'])


def test_full_model_eval_flag_needs_the_pre_stage():
  import full_model_eval
  assert full_model_eval.build_parser().parse_args([]).cityscapes_output is None
  with pytest.raises(rn.RecAttendError, match='--fg_model_id'):
    full_model_eval.main(['--model_id', 'm', '--results', 'nowhere', '--cityscapes_output', 'nowhere'])


# ---- no device, no result
def test_no_device_raises(monkeypatch):
  import torch
  import cityscapes_eval as ce
  import ra_ops as ops
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  y, s, sem = torch.zeros(1, 2, 8, 8), torch.ones(1, 2), torch.zeros(1, 4, 4, 9)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ce.label_instances(y, s, sem, (8, 8), [0.3])
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.instance_class_vote(y, sem)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.sem_foreground(sem, 8, 8)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.instance_class_pick(torch.zeros(1, 2, 9), s)


def test_argument_validation_without_gpu():
  lib = rn.lib()
  assert lib.ra_instance_class_vote_workspace_floats(1, 20, 1024, 2048, 9) == 1024 * 20 * 9
  assert lib.ra_instance_class_vote_workspace_floats(4, 20, 1024, 2048, 9) == 4 * 256 * 20 * 9
  assert lib.ra_instance_class_vote_workspace_floats(1, 2, 8, 8, 9) == 1 * 2 * 9
  assert lib.ra_instance_class_vote_f32(None, None, 1, 2, 8, 8, 4, 4, 9, None, None, 0, None, None, None, None) == rn.RA_E_INVALID
  one = 16  # any non-null address: the shape is refused before anything is read or launched
  for T, C in ((33, 9), (0, 9), (20, 1), (20, 17)):
    rc = lib.ra_instance_class_vote_f32(one, one, 1, T, 8, 8, 4, 4, C, None, one, 1 << 20, one, None, None, None)
    assert rc == rn.RA_E_SHAPE and b'ra_instance_class_vote_f32' in lib.ra_last_error_string()
  assert lib.ra_instance_class_vote_f32(one, one, 1, 2, 8, 8, 4, 4, 9, None, one, 3, one, None, None, None) == rn.RA_E_WORKSPACE
  assert lib.ra_instance_class_pick_f32(one, one, 1, 40, 9, one, one, None) == rn.RA_E_SHAPE
  assert lib.ra_sem_foreground_f32(one, 1, 4, 4, 17, 8, 8, 0.3, one, None) == rn.RA_E_SHAPE
  assert lib.ra_sem_foreground_f32(None, 1, 4, 4, 9, 8, 8, 0.3, None, None) == rn.RA_E_INVALID
