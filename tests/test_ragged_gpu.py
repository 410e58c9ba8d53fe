"""Mixed full sizes in one batch on the MI355X: the ragged entry points (ra_*_ragged_*) on six images of six sizes in one
flat buffer, in the three layouts of tests/ragged_cases.py, against every image ALONE.

Bars.  Instance evaluator: the band of tests/ins_eval_oracle.py per image (area_b equal, lo <= inter <= hi, inter equal to
the oracle's where the band is empty; the conditions share <= BAND_SHARE and ties == 0 are asserted).  Sweep: the band of
tests/test_fg_eval_gpu.py (DELTA, BAND_SHARE) per image.  Catalogue and labels: integer and double code built without
contraction, so EQUAL to the uniform entry point and to tests/labels_oracle.py on every image alone, every output.  In all
of them the three layouts give identical integers per image (the load width touches no arithmetic) and repeated runs
identical bits.  Whether the ragged evaluator equals the uniform entry point image by image is printed, not asserted: two
instantiations of float32 code, and the band is the bar."""
import ctypes

import numpy as np
import pytest
import torch

import ins_eval_oracle as ieo
import labels_oracle as lo
import ra_native as rn
import ra_ops as ops
import ragged_cases as rc
from test_fg_eval_gpu import BAND_SHARE, DELTA

pytestmark = pytest.mark.gpu
ORI_GUARD = 1e-6  # tests/test_labels_gpu.py


def _dev(a, dtype=None):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _packed(images, name, dtype):
  """(flat device tensor, geometry, batch order) of the listed images in the layout `name`."""
  order, align = rc.layout(name, len(images))
  geo, total = rc.geometry([images[i].shape for i in order], align)
  if name == 'aligned':  # the product's own packer gives this layout
    flat, g = ops.pack_ragged([images[i] for i in order], {np.int32: torch.int32, np.uint8: torch.uint8}[dtype])
    assert np.array_equal(g, geo) and flat.numel() == total and not (geo[:, 0] % 4).any()
    return flat, geo, order
  return _dev(rc.flatten([images[i] for i in order], geo, total, dtype)), geo, order


# ------------------------------------------------------------------------------------------------------------ instance evaluator
@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
def test_instance_eval_counts_ragged(cuda, morph, with_fg):
  n = len(rc.EVAL_SIZES)
  cases = [rc.ins_eval_image(i) for i in range(n)]
  yc = np.concatenate([c['yc'] for c in cases])
  inst = np.concatenate([c['inst_id'] for c in cases])
  for K in (1, 10, 16):
    thr = ieo.THRESHOLDS[K]
    per_layout = {}
    for name in rc.LAYOUTS:
      gt, geo, order = _packed([c['gt_ids'][0] for c in cases], name, np.int32)
      fg = _packed([c['fg'][0] for c in cases], name, np.uint8)[0] if with_fg else None
      args = (_dev(yc[order]), gt, geo, _dev(inst[order]), thr)
      runs = [ops.instance_eval_counts_ragged(*args, fg_flat=fg, morph=morph) for _ in range(3)]
      for inter, area_b in runs[1:]:  # integer atomics: the same bits on every run
        assert torch.equal(inter, runs[0][0]) and torch.equal(area_b, runs[0][1])
      per_layout[name] = (rc.unpermute(order, runs[0][0].cpu().numpy()).astype(np.int64),
                          rc.unpermute(order, runs[0][1].cpu().numpy()).astype(np.int64))
    inter, area_b = per_layout['packed']
    for name in rc.LAYOUTS[1:]:
      assert (per_layout[name][0] == inter).all() and (per_layout[name][1] == area_b).all(), name
    for i, c in enumerate(cases):
      lo_, hi_, share, ties, ref_inter, ref_area = rc.ins_eval_reference(i, K, with_fg, morph)
      assert share <= ieo.BAND_SHARE and ties == 0  # conditions on the inputs
      alone = ops.instance_eval_counts(_dev(c['yc']), _dev(c['gt_ids']), _dev(c['inst_id']), thr,
                                       fg=_dev(c['fg']) if with_fg else None, morph=morph)
      same = bool((alone[0].cpu().numpy()[0] == inter[i]).all() and (alone[1].cpu().numpy()[0] == area_b[i]).all())
      print('image %d %s morph %d fg %d K %2d: band of %d counts (share %.5f); ragged differs from the float64 counts in %d entries; '
            'ragged == the uniform entry point on the image alone: %s' % (i, rc.EVAL_SIZES[i], morph, with_fg, K, int((hi_ - lo_).sum()),
                                                                         share, int((inter[i] != ref_inter[0]).sum()), same))
      assert (area_b[i] == ref_area[0]).all()
      assert (lo_[0] <= inter[i]).all() and (inter[i] <= hi_[0]).all()
      if (lo_ == hi_).all():
        assert (inter[i] == ref_inter[0]).all()


# ------------------------------------------------------------------------------------------------------------------------- sweep
def test_fg_sweep_counts_ragged(cuda):
  n = len(rc.EVAL_SIZES)
  imgs = [rc.sweep_image(i) for i in range(n)]
  src = np.concatenate([s for s, _, _ in imgs])
  thr = rc.SWEEP_THRESHOLDS
  got = {}
  for name in rc.LAYOUTS:
    gt, geo, order = _packed([g[0] for _, _, g in imgs], name, np.uint8)
    runs = [ops.fg_sweep_counts_ragged_device(_dev(src[order]), gt, geo, thr).cpu().numpy() for _ in range(3)]
    assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all()
    c = ops.fg_sweep_counts_ragged(_dev(src[order]), gt, geo, thr)
    assert c['pixels'].tolist() == [rc.EVAL_SIZES[i][0] * rc.EVAL_SIZES[i][1] for i in order] and c['count_a'].dtype == np.int64
    got[name] = tuple(rc.unpermute(order, c[k]) for k in ('count_a', 'sum_ab', 'sum_b'))
    assert (runs[0][:, :10] == c['count_a']).all() and not runs[0][:, 10:16].any() and not runs[0][:, 26:32].any()
  for name in rc.LAYOUTS[1:]:
    for a, b in zip(got['packed'], got[name]):
      assert (a == b).all(), name
  count_a, sum_ab, sum_b = got['packed']
  for i in range(n):
    lo_, hi_, inside = rc.sweep_band(i, DELTA)
    share = inside.max() / float(rc.EVAL_SIZES[i][0] * rc.EVAL_SIZES[i][1])
    print('image %d %s: at most %d pixels inside the band (share %.2e)' % (i, rc.EVAL_SIZES[i], inside.max(), share))
    assert share <= BAND_SHARE  # a condition on the inputs
    assert (lo_[0][0] <= count_a[i]).all() and (count_a[i] <= hi_[0][0]).all()
    assert (lo_[1][0] <= sum_ab[i]).all() and (sum_ab[i] <= hi_[1][0]).all()
    assert sum_b[i] == lo_[2][0]
    s, _, g = imgs[i]
    alone = ops.fg_sweep_counts(_dev(s), _dev(g), thr)
    print('    ragged == the uniform entry point on the image alone: %s' % bool(
        (alone['count_a'][0] == count_a[i]).all() and (alone['sum_ab'][0] == sum_ab[i]).all()))


# --------------------------------------------------------------------------------------------------------- catalogue and labels
def _label_batch(dataset, name, images=None):
  images = [rc.label_image(i, dataset) for i in range(len(rc.LABEL_SIZES))] if images is None else images
  gt, geo, order = _packed(images, name, np.int32)
  return images, gt, geo, order


@pytest.mark.parametrize('dataset', [lo.PLAIN, lo.CITYSCAPES], ids=['plain', 'cityscapes'])
def test_catalogue_and_labels_ragged(cuda, dataset):
  rule = 'cityscapes' if dataset == lo.CITYSCAPES else 'kitti'
  H, W, T = rc.LABEL_H, rc.LABEL_W, rc.LABEL_T
  first = None
  for name in rc.LAYOUTS:
    images, gt, geo, order = _label_batch(dataset, name)
    cat = ops.gt_instance_catalog_ragged(gt, geo)
    got = ops.assemble_labels_ragged(gt, geo, H, W, T, rule, want=ops.LABEL_OUTPUTS)
    again = ops.assemble_labels_ragged(gt, geo, H, W, T, rule, want=ops.LABEL_OUTPUTS)
    fg_flat = got['fg_gt_full'].cpu().numpy()
    covered = np.zeros(fg_flat.shape, bool)
    for b, i in enumerate(order):
      img = images[i]
      ref = rc.label_reference(i, dataset)
      assert ref['ori_margin'] >= ORI_GUARD  # a condition on the input
      d = _dev(img[None])
      u_cat = ops.gt_instance_catalog(d)
      uni = ops.assemble_labels(d, H, W, T, rule, want=ops.LABEL_OUTPUTS)
      for k in range(3):  # ids, pixels, count
        assert torch.equal(cat[k][b], u_cat[k][0]), (name, i, k)
      vals, cnts = np.unique(img, return_counts=True)
      assert cat[0][b, :len(vals)].cpu().tolist() == vals.tolist() and cat[1][b, :len(vals)].cpu().tolist() == cnts.tolist()
      off, h, w = geo[b].tolist()
      covered[off:off + h * w] = True
      for key in lo.KEYS:
        g = fg_flat[off:off + h * w].reshape(h, w) if key == 'fg_gt_full' else got[key][b].cpu().numpy()
        r, u = ref[key][0], uni[key][0].cpu().numpy()
        assert g.dtype == r.dtype and g.shape == r.shape, (name, i, key, g.dtype, r.dtype, g.shape, r.shape)
        assert np.array_equal(g, r), (name, i, key, 'oracle')
        assert np.array_equal(g, u), (name, i, key, 'uniform entry point')
    assert not fg_flat[~covered].any()  # the gaps between images are not written
    for key in ops.LABEL_OUTPUTS:
      assert torch.equal(got[key], again[key]), (name, key)
    dense = {k: rc.unpermute(order, got[k].cpu().numpy()) for k in lo.KEYS if k != 'fg_gt_full'}
    if first is None:
      first = dense
    for k in dense:
      assert np.array_equal(dense[k], first[k]), (name, k)


def test_an_overflowing_image_spares_its_neighbours(cuda):
  """Image 1 (16 x 128) holds 257 distinct ids: its status word says so, assemble_labels_ragged names it, and every other
  image of the batch equals its reference."""
  images = [rc.label_image(i, lo.PLAIN) for i in range(len(rc.LABEL_SIZES))]
  many = np.zeros_like(images[1])
  many.reshape(-1)[:257] = np.arange(1, 258)
  images[1] = many
  H, W, T = rc.LABEL_H, rc.LABEL_W, rc.LABEL_T
  for name in ('packed', 'aligned'):
    _, gt, geo, order = _label_batch(lo.PLAIN, name, images)
    ids, pixels, count, status = ops.gt_instance_catalog_ragged(gt, geo, check_status=False)
    assert status.cpu().tolist() == [0, rn.RA_GT_STATUS_COUNT, 0, 0, 0, 0]
    got = ops.assemble_labels_ragged_raw(gt, geo, (ids, pixels, count), H, W, T, 'kitti')
    for b in (0, 2, 3, 4, 5):
      ref = rc.label_reference(b, lo.PLAIN)
      off, h, w = geo[b].tolist()
      for key in lo.KEYS:
        g = got[key][off:off + h * w].view(h, w) if key == 'fg_gt_full' else got[key][b]
        assert np.array_equal(g.cpu().numpy(), ref[key][0]), (name, b, key)
    with pytest.raises(rn.RecAttendError, match=r'image b\.png has more than 256 distinct instance ids'):
      ops.assemble_labels_ragged(gt, geo, H, W, T, 'kitti', names=['a.png', 'b.png', 'c.png', 'd.png', 'e.png', 'f.png'])


# --------------------------------------------------------------------------------------------------------------------- refusals
def _table(rows):
  return (rn.ImageGeo * len(rows))(*[rn.ImageGeo(*r) for r in rows])


def test_refusals(cuda):
  """The C entry points on device memory: RA_E_SHAPE naming the image, nothing launched, the outputs (and the device table)
  keep what they held."""
  lib = rn.lib()
  c = rc.ins_eval_image(0)  # 37 x 50
  yc2 = _dev(np.concatenate([c['yc'], c['yc']]))
  inst2 = _dev(np.concatenate([c['inst_id'], c['inst_id']]))
  P = 2 * 37 * 50
  gt = _dev(np.concatenate([c['gt_ids'].reshape(-1)] * 2))
  gt8 = gt.to(torch.uint8)
  thr = np.array([0.3], np.float32)
  bad = {'overlapping': ([(0, 37, 50), (1849, 37, 50)], P, r'image 1 starts at element 1849, inside image 0'),
         'past total': ([(0, 37, 50), (1850, 37, 50)], P - 1, r'image 1 .* beyond the buffer'),
         'zero-sized': ([(0, 37, 50), (1850, 0, 50)], P, r'image 1 is 0 x 50'),
         'negative': ([(0, 37, 50), (1850, 37, -1)], P, r'image 1 is 37 x -1')}
  gdev = torch.full((4,), 7, dtype=torch.int64, device='cuda')
  inter = torch.full((2, 1, 4, 5), 7, dtype=torch.int32, device='cuda')
  area = torch.full((2, 4), 7, dtype=torch.int32, device='cuda')
  counts = torch.full((2, rn.RA_FG_SWEEP_SLOTS), 7, dtype=torch.int64, device='cuda')
  cat = [torch.full((2, ops.MAX_GT), 7, dtype=torch.int32, device='cuda') for _ in range(2)] + \
        [torch.full((2,), 7, dtype=torch.int32, device='cuda') for _ in range(2)]
  ws = torch.zeros((1 << 16,), dtype=torch.int64, device='cuda')
  y_gt = torch.full((2, 3, 4, 6), 7, dtype=torch.float32, device='cuda')
  fg_full = torch.full((P,), 7, dtype=torch.uint8, device='cuda')
  outs = [gdev, inter, area, counts, y_gt, fg_full] + cat

  def untouched():
    torch.cuda.synchronize()
    return all(int(t.min()) == 7 and int(t.max()) == 7 for t in outs)

  def err():
    return lib.ra_last_error_string().decode()

  import re
  for what, (rows, total, pattern) in bad.items():
    tab = _table(rows)
    calls = {
        'eval': lambda: lib.ra_instance_eval_counts_ragged_f32(yc2.data_ptr(), gt.data_ptr(), inst2.data_ptr(), None, total, tab,
                                                               gdev.data_ptr(), 2, 4, 8, 12, 0, thr.ctypes.data, 1, inter.data_ptr(),
                                                               area.data_ptr(), rn.stream_ptr()),
        'sweep': lambda: lib.ra_fg_sweep_counts_ragged_f32(yc2.data_ptr(), gt8.data_ptr(), total, tab, gdev.data_ptr(), 2, 8, 12,
                                                           thr.ctypes.data, 1, counts.data_ptr(), rn.stream_ptr()),
        'catalogue': lambda: lib.ra_gt_instance_catalog_ragged_i32(gt.data_ptr(), total, tab, gdev.data_ptr(), 2, ws.data_ptr(),
                                                                   2 * ws.numel(), cat[0].data_ptr(), cat[1].data_ptr(),
                                                                   cat[2].data_ptr(), cat[3].data_ptr(), rn.stream_ptr()),
        'labels': lambda: lib.ra_labels_assemble_ragged_i32(gt.data_ptr(), total, tab, gdev.data_ptr(), cat[0].data_ptr(),
                                                            cat[2].data_ptr(), 2, 4, 6, 3, rn.RA_LABELS_PLAIN, ws.data_ptr(),
                                                            8 * ws.numel(), None, None, None, None, None, y_gt.data_ptr(), None, None,
                                                            None, fg_full.data_ptr(), rn.stream_ptr())}
    for entry, call in calls.items():
      rcode = call()
      assert rcode == rn.RA_E_SHAPE and re.search(pattern, err()), (what, entry, rcode, err())
      assert untouched(), (what, entry)
  # an image over 2^24 pixels: the evaluator's own bound (the table alone is looked at; no such buffer is needed)
  tab = _table([(0, 37, 50), (1852, 4097, 4096)])
  rcode = lib.ra_instance_eval_counts_ragged_f32(yc2.data_ptr(), gt.data_ptr(), inst2.data_ptr(), None, 1852 + 4097 * 4096, tab,
                                                 gdev.data_ptr(), 2, 4, 8, 12, 0, thr.ctypes.data, 1, inter.data_ptr(), area.data_ptr(),
                                                 rn.stream_ptr())
  assert rcode == rn.RA_E_SHAPE and re.search(r'image 1 is 4097 x 4096 \(h \* w <= 2\^24', err()) and untouched()
  # a network size above one image's full size
  tab = _table([(0, 37, 50), (1850, 37, 50)])
  for H, W in ((38, 6), (4, 51)):
    rcode = lib.ra_labels_assemble_ragged_i32(gt.data_ptr(), P, tab, gdev.data_ptr(), cat[0].data_ptr(), cat[2].data_ptr(), 2, H, W, 3,
                                              rn.RA_LABELS_PLAIN, ws.data_ptr(), 8 * ws.numel(), None, None, None, None, None,
                                              y_gt.data_ptr(), None, None, None, fg_full.data_ptr(), rn.stream_ptr())
    assert rcode == rn.RA_E_SHAPE and re.search(r'image 0 is 37 x 50, below the network size %d x %d' % (H, W), err()) and untouched()
  # the wrappers: the same refusals as exceptions, and their own checks
  geo = np.array([(0, 37, 50), (1849, 37, 50)], np.int64)
  with pytest.raises(rn.RecAttendError, match='image 1 starts at element 1849'):
    ops.instance_eval_counts_ragged(yc2, gt, geo, inst2, [0.3])
  with pytest.raises(rn.RecAttendError, match='image 1 starts at element 1849'):
    ops.fg_sweep_counts_ragged(yc2[:, 0].contiguous(), gt8, geo, [0.3])
  with pytest.raises(rn.RecAttendError, match='image 1 starts at element 1849'):
    ops.gt_instance_catalog_ragged(gt, geo)
  geo[1, 0] = 1850
  with pytest.raises(rn.RecAttendError, match='below the network size 38 x 6'):
    ops.assemble_labels_ragged(gt, geo, 38, 6, 3, 'kitti')
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts_ragged(yc2.cpu(), gt, geo, inst2, [0.3])
  with pytest.raises(rn.RecAttendError, match=r'\[B,3\]'):
    ops.gt_instance_catalog_ragged(gt, geo[:, :2])
  with pytest.raises(rn.RecAttendError, match='for the geometry\'s 2 images'):
    ops.instance_eval_counts_ragged(yc2[:1].contiguous(), gt, geo, inst2[:1].contiguous(), [0.3])
  with pytest.raises(rn.RecAttendError, match='>= 0'):
    ops.instance_eval_counts_ragged(yc2, gt, geo, inst2, [0.3, -0.01])
  assert ctypes.sizeof(rn.ImageGeo) == 16
