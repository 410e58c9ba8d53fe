"""Float64 NumPy restatement of the reference's label stage, written from those lines and in ITS formulation — a list of
full-size masks, each resized on its own, the orientation over the stack, the sort by area — not the kernels' (sample the
id image, compare ids): data_api/sep_labels.py, data_api/cvppp.py:49-63 / kitti.py:51-65 / cityscapes.py:88-119,
data_api/ins_seg_assembler.py:120-151, data_api/orientation.py:31-85, data_api/ins_seg_dataset.py:158-172,216-236,257-271,
fg_model_eval.py:142-143.  The test helper of test_labels*.py and the host stand-in tools/labels_bench.py times.  Two of the
reference's modules run once translated to Python 3, orientation.py and sep_labels.py: oracle/toolkit_fixtures.py recorded
get_orientation ('class' and 'one_hot') and get_separate_labels on ellipse images and on hand-made edge masks as
tests/golden/toolkit_orientation.npz, and tests/test_toolkit_fixtures.py holds get_orientation / separate_labels here to
them (every class equal).  The rest of the stage (the dataset classes, the assembler: cv2, h5py) still cannot be run.

Two statements are this project's and REMAIN UNCHECKED against the reference's libraries, cv2 being absent: the nearest-neighbour
rule is OpenCV's resizeNN restated from its source, and equal areas are ordered as a stable ascending sort read backwards
(NumPy's default argsort is stable only up to 16 elements)."""
import numpy as np

from cs_oracle import LABELS  # [(name, label id)]: the eight Cityscapes labels with instances, in trainId order

PLAIN, CITYSCAPES = 0, 1
NUM_ORI = 8


def nn_index(n_dst, n_src):
  """cv2.resize(..., INTER_NEAREST): destination index d reads min(floor(d * (1 / (n_dst / n_src))), n_src - 1)."""
  scale = 1.0 / (float(n_dst) / float(n_src))
  return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * scale).astype(np.int64), n_src - 1)


def resize_nn(img, H, W):
  return img[nn_index(H, img.shape[0])][:, nn_index(W, img.shape[1])]


def separate_labels(label_img):
  """sep_labels.get_separate_labels on a one-channel image: ([full-size uint8 masks], [ids]) of every id != 0, ascending."""
  colors = np.unique(label_img)
  return [(label_img == c).astype(np.uint8) for c in colors if c != 0], [int(c) for c in colors if c != 0]


def get_segmentations(label_img, dataset):
  """get_segmentations of the dataset classes: (masks, ids, semantic class per mask, [per-class full-size union or None])."""
  segm, colors = separate_labels(label_img)
  if dataset == PLAIN:
    union = np.zeros(label_img.shape, np.uint8)
    for ss in segm:
      union = np.maximum(union, ss)
    return segm, colors, [0] * len(segm), [union]
  train_id = {label: k + 1 for k, (_, label) in enumerate(LABELS)}  # every other label's trainId is 0 or negative
  sem_segm = [None] * len(LABELS)
  out, ids, cls = [], [], []
  for ss, cc in zip(segm, colors):
    if cc > 1000:
      tid = train_id.get(int(np.floor(cc / 1000)), 0)
      if tid > 0:
        out.append(ss)
        ids.append(cc)
        cls.append(tid - 1)
        sem_segm[tid - 1] = ss.copy() if sem_segm[tid - 1] is None else np.maximum(sem_segm[tid - 1], ss)
  return out, ids, cls, sem_segm


def get_orientation(y):
  """orientation.get_orientation(y, encoding='class') for y [T,H,W] of 0 / 1 (B = 1 dropped; :51's expand_dims is taken on
  the last axis, as it was meant): (class uint8 [H,W], pre [T,H,W] = the value :72-73 floors, per instance)."""
  y = np.asarray(y, np.float64)
  T, H, W = y.shape
  idx_map = np.zeros((H, W, 2))
  idx_map[:, :, 0] += np.arange(H).reshape(-1, 1)
  idx_map[:, :, 1] += np.arange(W).reshape(1, -1)
  y2 = y[..., None]
  y_map = idx_map[None] * y2
  y_sum = y.sum(axis=1).sum(axis=1)[:, None] + 1e-7
  centroids = (y_map.sum(axis=1).sum(axis=1) / y_sum).reshape(T, 1, 1, 2)
  ovec = (y_map - centroids) * y2
  ovec = (ovec + 1e-8) / (np.sqrt((ovec * ovec).sum(axis=-1, keepdims=True)) + 1e-7)
  angle = np.arcsin(ovec[..., 0])
  xpos = (ovec[..., 1] > 0).astype('float')
  ypos = (ovec[..., 0] > 0).astype('float')
  angle = angle * xpos * ypos + (np.pi - angle) * (1 - xpos) * ypos + angle * xpos * (1 - ypos) + \
      (-np.pi - angle) * (1 - xpos) * (1 - ypos)
  angle = angle + np.pi / 8
  pre = (angle + np.pi) * NUM_ORI / 2 / np.pi
  angle_class = np.mod(np.floor(pre), NUM_ORI)
  return (angle_class * y).max(axis=0).astype('uint8'), pre


def assemble_image(label_img, H, W, T, dataset):
  """One image [Hf,Wf] of ids -> dict of what the stage writes for it, plus 'ori_margin': the least distance of the
  pre-floor orientation value from an integer over the foreground pixels (inf without any)."""
  label_img = np.asarray(label_img)
  segm, ids, cls, sem_segm = get_segmentations(label_img, dataset)
  num_obj = len(segm)
  small = [resize_nn(ss, H, W) for ss in segm]  # ins_seg_assembler.py:125
  d_cls = np.zeros((H, W), np.uint8)
  margin = np.inf
  if num_obj:
    stack = np.stack(small)
    d_cls, pre = get_orientation(stack)  # :136-139, over ALL instances
    on = stack > 0
    if on.any():
      margin = float(np.abs(pre[on] - np.round(pre[on])).min())
  area = np.array([yy.astype(np.float32).sum() for yy in small])  # ins_seg_dataset.py:169
  order = np.argsort(area, kind='stable')[::-1] if num_obj else np.zeros((0,), np.int64)
  y_gt = np.zeros((T, H, W), np.float32)
  s_gt = np.zeros((T,), np.float32)
  inst_id, ar, sem = np.full((T,), -1, np.int32), np.zeros((T,), np.int32), np.full((T,), -1, np.int32)
  for jj in range(min(num_obj, T)):  # :171-172
    k = order[jj]
    y_gt[jj], inst_id[jj], ar[jj], sem[jj] = small[k], ids[k], int(area[k]), cls[k]
  s_gt[:min(num_obj, T)] = 1.0  # :267-271
  nsc = len(sem_segm)
  c_gt = np.zeros((H, W, nsc + 1 if nsc > 1 else 1), np.float32)
  if nsc > 1:  # :216-236
    for jj, ss in enumerate(sem_segm):
      if ss is not None:
        c_gt[:, :, jj + 1] = resize_nn(ss, H, W)  # ins_seg_assembler.py:145
    c_gt[:, :, 0] = 1 - c_gt.max(axis=2)
  else:
    c_gt[:, :, 0] = resize_nn(sem_segm[0], H, W)
  d_gt = np.stack([(d_cls == oo).astype(np.float32) for oo in range(NUM_ORI)], axis=-1)  # :257-262
  fg = np.zeros(label_img.shape, np.uint8)
  for ss in segm:  # fg_model_eval.py:142-143
    fg += ss
  return {'num_obj': np.int32(num_obj), 's_gt': s_gt, 'inst_id': inst_id, 'area': ar, 'sem_cls': sem, 'y_gt': y_gt,
          'd_cls': d_cls, 'd_gt': d_gt, 'c_gt': c_gt, 'fg_gt_full': fg, 'ori_margin': margin}


KEYS = ('num_obj', 's_gt', 'inst_id', 'area', 'sem_cls', 'y_gt', 'd_cls', 'd_gt', 'c_gt', 'fg_gt_full')


def assemble(gt_ids, H, W, T, dataset):
  """gt_ids [B,Hf,Wf] -> {key: stacked array} over KEYS, and 'ori_margin' = the least margin over the batch."""
  per = [assemble_image(img, H, W, T, dataset) for img in np.asarray(gt_ids)]
  out = {k: np.stack([p[k] for p in per]) for k in KEYS}
  out['ori_margin'] = min(p['ori_margin'] for p in per)
  return out


# ---- test inputs
def ellipse_ids(rng, B, Hf, Wf, n_inst, dataset=PLAIN, min_axis=0.08, max_axis=0.3):
  """int32 [B,Hf,Wf]: n_inst random ellipses per image, later ones painted over earlier ones; ids are 1 .. n_inst under
  PLAIN and label * 1000 + k over the eight instance labels, two stuff ids (7, 21) and one caravan (29000 + k) under
  CITYSCAPES."""
  rr, cc = np.mgrid[0:Hf, 0:Wf]
  gt = np.zeros((B, Hf, Wf), np.int32)
  for b in range(B):
    if dataset == CITYSCAPES:
      gt[b, : Hf // 3] = 21
      gt[b, Hf - Hf // 4:] = 7
    for k in range(n_inst):
      ry, rx = rng.uniform(min_axis, max_axis) * Hf, rng.uniform(min_axis, max_axis) * Wf
      cy, cx = rng.uniform(0, Hf), rng.uniform(0, Wf)
      if dataset == CITYSCAPES:
        label = 29 if k == 1 else LABELS[rng.randint(len(LABELS))][1]
        ident = label * 1000 + k
      else:
        ident = k + 1
      gt[b][((rr - cy) / ry) ** 2 + ((cc - cx) / rx) ** 2 <= 1.0] = ident
  return gt
