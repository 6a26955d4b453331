"""The per-sample training transforms of pointcept/datasets/transform.py on the device, under the reference's names and
constructor signatures (``TRANSFORMS.build(dict(type="RandomRotate", axis="z", ...))``), for dicts of GPU tensors.

Two things differ from the reference by design:

* **Draw and apply are separate.**  ``draw(rng, data_dict) -> params`` takes every random decision of one call from a
  ``numpy.random.Generator`` (owned by ``Compose``; no global ``random`` / ``np.random`` state, no device sync) and returns a
  small plain dict: fired flag, angle, scale, flips, blend, translation, a 64-bit seed for per-point noise.  ``apply(data_dict,
  params)`` does the work, ``__call__`` is ``apply(draw(...))``.  Replaying recorded parameters (``noise=`` / ``idx=`` entries
  replace a seed) makes every op comparable with the reference although the device draws its own numbers.
* **Compose fuses.**  A run of CenterShift / RandomRotate / RandomRotateTargetAngle / RandomScale / RandomShift / RandomFlip /
  RandomJitter is folded on the host into one fp64 affine ``A x + b``, one rotation quaternion, a reflection and a scale factor and
  applied in ONE ``ss_aug_gaussians`` pass over coord / quat / scale / normal.  Ops that need the bounding box of the *current*
  coordinates (CenterShift, rotations with ``center=None``) call ``ss_aug_bbox`` with the pending affine: that is a 6-float
  device -> host readback (a sync) per such op, and no pass over memory is spent on flushing.  The pass is flushed at the first
  op outside the family, when a rotation follows a flip or a jitter (the kernel rotates first), or when a second flip or jitter
  arrives.  A run of ChromaticAutoContrast / ChromaticTranslation / ChromaticJitter / NormalizeColor in that order is one
  ``ss_aug_color`` pass.  ``Compose(fuse=False)`` runs op by op.

``pc_coord`` / ``pc_segment`` (the point cloud some val / test lists carry beside the Gaussians) follow the reference: CenterShift, the
rotations, RandomScale and RandomFlip move the cloud with the Gaussians (a second pending affine, one more ``ss_aug_gaussians`` launch
per flush), ``GridSample(apply_to_pc=True)`` keeps one point per occupied cell of the cloud's own grid, every other op passes both keys through.

All ops work IN PLACE on float32 contiguous tensors (as the reference mutates its arrays) and refuse CPU tensors: there is no
CPU fallback.  ``draw``, the host composition (``RigidState`` with a ``bbox_fn``) and ``box_blur3`` need no device.
"""
import numpy as np
import torch

from .. import gpu_transforms as gt
from .. import native as nv
from .registry import TRANSFORMS


# ---- host quaternion helpers (fp64, wxyz) ---------------------------------------------------------------------------------------
def quat_mul(p, q):
    """Hamilton product p (x) q, wxyz."""
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.array([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], dtype=np.float64)


def quat_from_matrix(m):
    """Rotation matrix -> unit quaternion (wxyz) with the sign scipy's Rotation.from_matrix gives: the branch is the arg-max of
    [M00, M11, M22, trace] and the component it selects (x / y / z / w) comes out positive."""
    m = np.asarray(m, dtype=np.float64)
    dec = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
    c = int(np.argmax(dec))
    q = np.empty(4)                                           # xyzw while it is built
    if c != 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - dec[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    else:
        q[0] = m[2, 1] - m[1, 2]
        q[1] = m[0, 2] - m[2, 0]
        q[2] = m[1, 0] - m[0, 1]
        q[3] = 1 + dec[3]
    q /= np.linalg.norm(q)
    return np.array([q[3], q[0], q[1], q[2]])


def axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    if axis == "z":
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    raise NotImplementedError("axis must be 'x', 'y' or 'z'")


def box_blur3(noise, rounds=2):
    """ElasticDistortion's smoothing (transform.py:1135-1154): the 3-tap box blur (1/3, 1/3, 1/3) along x, then y, then z with
    zero padding, `rounds` times, on a (d0, d1, d2, C) float32 tensor of any device."""
    third = noise.new_tensor(1.0 / 3.0)
    for _ in range(rounds):
        for dim in (0, 1, 2):
            pad = torch.zeros_like(noise.narrow(dim, 0, 1))
            ext = torch.cat([pad, noise, pad], dim=dim)
            d = noise.shape[dim]
            noise = (ext.narrow(dim, 0, d) + ext.narrow(dim, 1, d) + ext.narrow(dim, 2, d)) * third
    return noise


def _seed(rng):
    return int(rng.integers(0, 1 << 63))


def _dev(t, name, cols=None):
    """The tensors the kernels update in place: float32, contiguous, on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: scenesplat_amd transforms need a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name}: must be a contiguous float32 tensor (it is updated in place)")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise RuntimeError(f"{name}: expected (n, {cols}), got {tuple(t.shape)}")
    return t


def _has_pc(data_dict):
    """the reference treats pc_coord inside its `if "coord" in data_dict` branches: both keys, or the cloud is left alone"""
    return "coord" in data_dict and "pc_coord" in data_dict


def _noise_arg(noise, like):
    """A recorded (n, 3) N(0,1) array / tensor -> float32 device tensor."""
    if noise is None:
        return None
    return torch.as_tensor(np.asarray(noise, dtype=np.float32) if not isinstance(noise, torch.Tensor) else noise,
                           dtype=torch.float32).to(like.device).contiguous()


# ---- the pending rigid transform ------------------------------------------------------------------------------------------------
class RigidState:
    """What a run of rigid ops has folded so far: coord -> A x + b (fp64), quaternion -> q (x) quat then the flip conjugation,
    scale -> scale * smul, normal -> L normal, then the jitter.  bbox_fn(A, b) -> 6 floats overrides the device bounding box
    (host-only composition: tests, dry runs).
    pc_coord (the point cloud some lists carry beside the Gaussians) -> A_pc x + b_pc: the ops that treat it in the reference
    (CenterShift, the rotations, RandomScale, RandomFlip) fold into it with `pc=True`, with the Gaussians' shift and centre;
    RandomShift and RandomJitter do not, so the two affines differ after them.  The flush rules are shared."""
    family = "rigid"

    def __init__(self, bbox_fn=None):
        self.bbox_fn = bbox_fn
        self.reset()

    def reset(self):
        self.A, self.b, self.L = np.eye(3), np.zeros(3), np.eye(3)
        self.A_pc, self.b_pc = np.eye(3), np.zeros(3)
        self.q = None                 # composed rotation quaternion (wxyz), None = no rotation yet
        self.flip = 0                 # bit 0: x, bit 1: y
        self.smul = np.ones(3)
        self.scaled = False
        self.jitter = None            # dict(sigma, clip, seed | noise)

    def coord_pending(self):
        return not (np.array_equal(self.A, np.eye(3)) and not self.b.any())

    def affine12(self):
        return None if not self.coord_pending() else list(self.A.reshape(-1)) + list(self.b)

    def pc_pending(self):
        return not (np.array_equal(self.A_pc, np.eye(3)) and not self.b_pc.any())

    def affine12_pc(self):
        return None if not self.pc_pending() else list(self.A_pc.reshape(-1)) + list(self.b_pc)

    def bbox(self, data):
        """Bounding box {min xyz, max xyz} of the current coordinates, pending affine included (6-float readback)."""
        if self.jitter is not None:
            self.flush(data)
        if self.bbox_fn is not None:
            return np.asarray(self.bbox_fn(self.A, self.b), dtype=np.float64)
        return nv.aug_bbox(_dev(data["coord"], "coord", 3), self.affine12()).cpu().numpy().astype(np.float64)

    def before_coord_op(self, data):
        if self.jitter is not None:           # the kernel adds the jitter last
            self.flush(data)

    def shift(self, data, t, pc=False):
        self.before_coord_op(data)
        self.b = self.b + np.asarray(t, dtype=np.float64)
        if pc:
            self.b_pc = self.b_pc + np.asarray(t, dtype=np.float64)

    def rotate(self, data, rot, center, has_coord, pc=False):
        if self.flip or self.jitter is not None:          # the kernel rotates before it flips
            self.flush(data)
        if has_coord:
            if center is None:
                bb = self.bbox(data)
                center = (bb[:3] + bb[3:]) / 2
            center = np.asarray(center, dtype=np.float64)
            self.A = rot @ self.A
            self.b = rot @ (self.b - center) + center
            if pc:                                        # about the SAME centre: the Gaussians' (transform.py:577-580)
                self.A_pc = rot @ self.A_pc
                self.b_pc = rot @ (self.b_pc - center) + center
        self.L = rot @ self.L
        r = quat_from_matrix(rot)
        self.q = r if self.q is None else quat_mul(r, self.q)

    def scale(self, data, s, pc=False):
        self.before_coord_op(data)
        s = np.broadcast_to(np.asarray(s, dtype=np.float64), (3,))
        self.A = s[:, None] * self.A
        self.b = s * self.b
        if pc:
            self.A_pc = s[:, None] * self.A_pc
            self.b_pc = s * self.b_pc
        self.smul = self.smul * s
        self.scaled = True

    def reflect(self, data, flip_x, flip_y, pc=False):
        if not (flip_x or flip_y):
            return
        if self.flip or self.jitter is not None:          # one conjugation + sign rule per pass
            self.flush(data)
        f = np.array([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
        self.A = f[:, None] * self.A
        self.b = f * self.b
        self.L = f[:, None] * self.L
        if pc:
            self.A_pc = f[:, None] * self.A_pc
            self.b_pc = f * self.b_pc
        self.flip = (1 if flip_x else 0) | (2 if flip_y else 0)

    def add_jitter(self, data, sigma, clip, seed=0, noise=None):
        if self.jitter is not None:
            self.flush(data)
        self.jitter = dict(sigma=sigma, clip=clip, seed=seed, noise=noise)

    def flush(self, data):
        """ONE ss_aug_gaussians pass over the arrays the pending ops touch, and one more over pc_coord when they touched the cloud."""
        aff, aff_pc = self.affine12(), self.affine12_pc()
        pc = _dev(data["pc_coord"], "pc_coord", 3) if aff_pc is not None and "pc_coord" in data else None
        coord = data.get("coord") if (aff is not None or self.jitter is not None) else None
        quat = data.get("quat") if (self.q is not None or self.flip) else None
        scale = data.get("scale") if self.scaled else None
        normal = data.get("normal") if not np.array_equal(self.L, np.eye(3)) else None
        j = self.jitter
        if coord is not None or quat is not None or scale is not None or normal is not None:
            nv.aug_gaussians_(
                coord=None if coord is None else _dev(coord, "coord", 3), quat=None if quat is None else _dev(quat, "quat", 4),
                scale=None if scale is None else _dev(scale, "scale", 3), normal=None if normal is None else _dev(normal, "normal", 3),
                affine=aff, rquat=None if self.q is None else list(self.q), flip=self.flip, scale_mul=list(self.smul),
                lin=list(self.L.reshape(-1)), jitter=None if j is None or coord is None else (j["sigma"], j["clip"]),
                noise=None if j is None or coord is None else _noise_arg(j["noise"], coord), seed=0 if j is None else j["seed"])
        if pc is not None:
            nv.aug_gaussians_(coord=pc, affine=aff_pc)
        self.reset()


class ColorState:
    """Pending colour steps in the kernel's order: contrast (1) -> translation (2) -> jitter (3) -> normalize (4)."""
    family = "color"

    def __init__(self):
        self.reset()

    def reset(self):
        self.stage, self.flags, self.normalize = 0, 0, False
        self.lo = self.hi = self.tr = self.noise = None
        self.blend, self.std, self.seed = 0.0, 0.0, 0

    def enter(self, data, stage):
        if self.stage >= stage:
            self.flush(data)
        self.stage = stage

    def flush(self, data):
        if (self.flags or self.normalize) and "color" in data:
            c = _dev(data["color"], "color", 3)
            nv.aug_color_(c, self.flags, self.lo, self.hi, self.blend, self.tr, self.std, _noise_arg(self.noise, c), self.seed,
                          self.normalize)
        self.reset()


_STATES = dict(rigid=RigidState, color=ColorState)


class Transform:
    """Base: draw() takes the random decisions, apply() does the work; ops with a `family` can also fold() into a pending pass."""
    family = None

    def draw(self, rng, data_dict):
        return {}

    def fold(self, state, data_dict, params):
        raise NotImplementedError

    def apply(self, data_dict, params):
        state = _STATES[self.family]()
        self.fold(state, data_dict, params)
        state.flush(data_dict)
        return data_dict

    def __call__(self, data_dict, rng=None):
        return self.apply(data_dict, self.draw(np.random.default_rng() if rng is None else rng, data_dict))


# ---- rigid family ---------------------------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class CenterShift(Transform):
    """transform.py:446-465: x, y to the centre of the bounding box, z to its floor (apply_z) or untouched; pc_coord gets the
    same shift (the Gaussians' box, not its own)."""
    family = "rigid"

    def __init__(self, apply_z=True):
        self.apply_z = apply_z

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            bb = state.bbox(data_dict)
            state.shift(data_dict, [-(bb[0] + bb[3]) / 2, -(bb[1] + bb[4]) / 2, -bb[2] if self.apply_z else 0.0],
                        pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomShift(Transform):
    family = "rigid"

    def __init__(self, shift=((-0.2, 0.2), (-0.2, 0.2), (0, 0))):
        self.shift = shift

    def draw(self, rng, data_dict):
        return dict(shift=[float(rng.uniform(lo, hi)) for lo, hi in self.shift])

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.shift(data_dict, params["shift"])


@TRANSFORMS.register_module()
class RandomRotate(Transform):
    """transform.py:544-601: rotates coord about `center` (None: the bounding-box centre of the current coordinates), the
    Gaussians' quaternions (left-multiplied) and the normals; pc_coord about the same centre."""
    family = "rigid"

    def __init__(self, angle=None, center=None, axis="z", always_apply=False, p=0.5):
        self.angle = [-1, 1] if angle is None else angle
        self.axis = axis
        self.always_apply = always_apply
        self.p = p if not self.always_apply else 1
        self.center = center
        axis_rotation(axis, 0.0)

    def draw(self, rng, data_dict):
        if rng.random() > self.p:
            return dict(fired=False)
        return dict(fired=True, angle=float(rng.uniform(self.angle[0], self.angle[1]) * np.pi))

    def fold(self, state, data_dict, params):
        if params["fired"]:
            state.rotate(data_dict, axis_rotation(self.axis, params["angle"]), self.center, "coord" in data_dict,
                         pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomRotateTargetAngle(RandomRotate):
    """transform.py:604-659: as RandomRotate with the angle taken from a list (multiples of pi)."""

    def __init__(self, angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75):
        super().__init__(angle=angle, center=center, axis=axis, always_apply=always_apply, p=p)

    def draw(self, rng, data_dict):
        if rng.random() > self.p:
            return dict(fired=False)
        return dict(fired=True, angle=float(rng.choice(np.asarray(self.angle, dtype=np.float64)) * np.pi))


@TRANSFORMS.register_module()
class RandomScale(Transform):
    """transform.py:662-678: coord, pc_coord and the Gaussians' `scale` are multiplied by the same draw."""
    family = "rigid"

    def __init__(self, scale=None, anisotropic=False):
        self.scale = scale if scale is not None else [0.95, 1.05]
        self.anisotropic = anisotropic

    def draw(self, rng, data_dict):
        return dict(scale=rng.uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1).tolist())

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.scale(data_dict, params["scale"], pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomFlip(Transform):
    """transform.py:681-727: mirrors x and / or y of coord, pc_coord and normal; the quaternions get the conjugation F R F."""
    family = "rigid"

    def __init__(self, p=0.5):
        self.p = p

    def draw(self, rng, data_dict):
        return dict(flip_x=bool(rng.random() < self.p), flip_y=bool(rng.random() < self.p))

    def fold(self, state, data_dict, params):
        state.reflect(data_dict, params["flip_x"], params["flip_y"], pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomJitter(Transform):
    """transform.py:730-745: coord += clip(sigma N(0,1), +-clip); params["noise"] (n, 3) replays recorded draws."""
    family = "rigid"

    def __init__(self, sigma=0.01, clip=0.05):
        assert clip > 0
        self.sigma = sigma
        self.clip = clip

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.add_jitter(data_dict, self.sigma, self.clip, params.get("seed", 0), params.get("noise"))


# ---- colour family --------------------------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class ChromaticAutoContrast(Transform):
    """transform.py:769-787; the per-channel lo / hi come from ss_aug_bbox on the colours (6-float readback)."""
    family = "color"

    def __init__(self, p=0.2, blend_factor=None):
        self.p = p
        self.blend_factor = blend_factor

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, blend=float(rng.random() if self.blend_factor is None else self.blend_factor))

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 1)
            bb = nv.aug_bbox(_dev(data_dict["color"], "color", 3)).cpu().numpy()
            if not (bb[3:] > bb[:3]).all():                   # the reference divides by hi - lo = 0 here and fills the channel with NaN
                raise ValueError("ChromaticAutoContrast: a colour channel is constant over the sample")
            state.lo, state.hi, state.blend = bb[:3].tolist(), bb[3:].tolist(), params["blend"]
            state.flags |= nv.AUG_COLOR_CONTRAST


@TRANSFORMS.register_module()
class ChromaticTranslation(Transform):
    """transform.py:790-800"""
    family = "color"

    def __init__(self, p=0.95, ratio=0.05):
        self.p = p
        self.ratio = ratio

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, tr=((rng.random(3) - 0.5) * 255 * 2 * self.ratio).tolist())

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 2)
            state.tr = list(params["tr"])
            state.flags |= nv.AUG_COLOR_TRANSLATE


@TRANSFORMS.register_module()
class ChromaticJitter(Transform):
    """transform.py:803-816; params["noise"] (n, 3) replays recorded draws."""
    family = "color"

    def __init__(self, p=0.95, std=0.005):
        self.p = p
        self.std = std

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, seed=_seed(rng))

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 3)
            state.std, state.seed, state.noise = self.std, params.get("seed", 0), params.get("noise")
            state.flags |= nv.AUG_COLOR_JITTER


@TRANSFORMS.register_module()
class NormalizeColor(Transform):
    """transform.py:415-420: color / 127.5 - 1"""
    family = "color"

    def fold(self, state, data_dict, params):
        if "color" in data_dict:
            state.enter(data_dict, 4)
            state.normalize = True


# ---- ops with a pass of their own -----------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class ElasticDistortion(Transform):
    """transform.py:1120-1178.  Per (granularity, magnitude) pair: bounding box of the current coordinates (6-float readback),
    a (dims, 3) N(0,1) grid smoothed by box_blur3, one ss_aug_elastic pass.  The grid's shape depends on the box the pass sees --
    the second pair sees the first one's output -- so draw() hands over the seed the grids are drawn from (host Generator, at
    apply time); params["noise"] = [raw grid per pair] replays recorded grids instead."""

    def __init__(self, distortion_params=None):
        self.distortion_params = [[0.2, 0.4], [0.8, 1.6]] if distortion_params is None else distortion_params

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < 0.95), seed=_seed(rng))

    @staticmethod
    def grid_geometry(bbox, granularity):
        """(noise_dim (3,) int, origin (3,) f32) from the fp32 box of the coordinates (transform.py:1138-1164)."""
        bb = np.asarray(bbox, dtype=np.float32)
        lo, hi = bb[:3], bb[3:]
        dim = np.floor_divide(hi - lo, np.float32(granularity)).astype(int) + 3
        return dim, lo - np.float32(granularity)

    def apply(self, data_dict, params):
        if "coord" not in data_dict or self.distortion_params is None or not params["fired"]:
            return data_dict
        coord = _dev(data_dict["coord"], "coord", 3)
        grids = params.get("noise")
        rng = None if grids is not None else np.random.default_rng(params["seed"])
        for k, (granularity, magnitude) in enumerate(self.distortion_params):
            dim, origin = self.grid_geometry(nv.aug_bbox(coord).cpu().numpy(), granularity)
            if grids is not None:
                raw = torch.as_tensor(np.asarray(grids[k], dtype=np.float32))
                if tuple(raw.shape) != (*dim.tolist(), 3):
                    raise ValueError(f"ElasticDistortion: recorded grid {tuple(raw.shape)} does not fit the box ({dim.tolist()})")
            else:
                raw = torch.from_numpy(rng.standard_normal((*dim.tolist(), 3), dtype=np.float32))
            noise = box_blur3(raw.to(coord.device)).contiguous()
            nv.aug_elastic_(coord, noise, origin.tolist(), granularity, magnitude)
        return data_dict


# the per-point entries RandomDropout subsets (transform.py:518-540)
DROPOUT_KEYS = ("coord", "color", "normal", "strength", "segment", "instance", "quat", "scale", "opacity", "lang_feat",
                "valid_feat_mask")


@TRANSFORMS.register_module()
class RandomDropout(Transform):
    """transform.py:497-541: keep int(n (1 - ratio)) random rows (randperm, unsorted as np.random.choice), of exactly the keys
    the reference subsets; `sampled_index` rows are always kept and remapped.  params["idx"] replays a recorded index."""

    def __init__(self, dropout_ratio=0.2, dropout_application_ratio=0.5):
        self.dropout_ratio = dropout_ratio
        self.dropout_application_ratio = dropout_application_ratio

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < self.dropout_application_ratio), seed=_seed(rng))

    def apply(self, data_dict, params):
        if not params["fired"]:
            return data_dict
        coord = data_dict["coord"]
        if not isinstance(coord, torch.Tensor) or not coord.is_cuda:
            raise RuntimeError("RandomDropout: GPU tensors required (no CPU fallback)")
        n = coord.shape[0]
        if params.get("idx") is not None:
            idx = torch.as_tensor(np.asarray(params["idx"]), dtype=torch.int64).to(coord.device)
        else:
            g = torch.Generator(device=coord.device)
            g.manual_seed(int(params["seed"]))
            idx = torch.randperm(n, device=coord.device, generator=g)[:int(n * (1 - self.dropout_ratio))]
        if "sampled_index" in data_dict:
            si = data_dict["sampled_index"].long()
            idx = torch.unique(torch.cat([idx, si]))
            mask = torch.zeros(n, dtype=torch.bool, device=coord.device)
            mask[si] = True
            data_dict["sampled_index"] = torch.nonzero(mask[idx]).reshape(-1)
        idx32 = idx.to(torch.int32).contiguous()
        for k in DROPOUT_KEYS:
            v = data_dict.get(k)
            if isinstance(v, torch.Tensor):
                data_dict[k] = gt.take_rows(v, idx32)
        return data_dict


@TRANSFORMS.register_module()
class ToTensor(Transform):
    """transform.py:374-399 for data that already lives in tensors: a pass-through (host arrays are the dataset's business)."""

    def apply(self, data_dict, params):
        return data_dict


@TRANSFORMS.register_module()
class Copy(Transform):
    """transform.py:355-371"""

    def __init__(self, keys_dict=None):
        self.keys_dict = dict(coord="origin_coord", segment="origin_segment") if keys_dict is None else keys_dict

    def apply(self, data_dict, params):
        import copy
        for key, value in self.keys_dict.items():
            if key in data_dict:
                v = data_dict[key]
                data_dict[value] = v.clone().detach() if isinstance(v, torch.Tensor) else copy.deepcopy(v)
        return data_dict


@TRANSFORMS.register_module()
class GridSample(Transform):
    """GridSample(mode="train") (transform.py:1181-1300) over gpu_transforms.grid_sample_train: one random point per occupied voxel,
    `keys` subset to it.  draw() hands the device generator its seed; params["idx"] replays a recorded per-voxel pick.
    `sampled_index` rows are always kept and remapped (as in RandomDropout).  With apply_to_pc, pc_coord / pc_segment are
    subset to one point per occupied cell of the cloud's own grid (gpu_transforms.grid_sample_pc), in ascending cell order --
    the reference emits the same rows in the order of its FNV hashes."""

    def __init__(self, grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"),
                 return_inverse=False, return_grid_coord=False, return_min_coord=False, return_displacement=False,
                 project_displacement=False, importance_sample_key=None, apply_to_pc=True):
        if mode != "train":
            raise NotImplementedError('GridSample: only mode="train" is registered (gpu_transforms.grid_sample_test serves the tester)')
        if return_min_coord or return_displacement or project_displacement or importance_sample_key is not None:
            raise NotImplementedError("GridSample: min_coord / displacement / importance sampling have no device form")
        self.grid_size, self.hash_type, self.mode, self.keys = grid_size, hash_type, mode, keys     # voxel keys are exact: no hash
        self.return_inverse, self.return_grid_coord, self.apply_to_pc = return_inverse, return_grid_coord, apply_to_pc

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def apply(self, data_dict, params):
        coord = data_dict["coord"]
        if not isinstance(coord, torch.Tensor) or not coord.is_cuda:
            raise RuntimeError("GridSample: GPU tensors required (no CPU fallback)")
        if "pc_coord" in data_dict and self.apply_to_pc:
            pc = _dev(data_dict["pc_coord"], "pc_coord", 3)
            seg = data_dict.get("pc_segment")
            if seg is not None and seg.shape[0] != pc.shape[0]:
                raise ValueError(f"GridSample: pc_segment has {seg.shape[0]} rows, pc_coord has {pc.shape[0]}")
            chosen = gt.grid_sample_pc(pc, self.grid_size, seg)
            data_dict["pc_coord"] = pc[chosen]
            if seg is not None:
                data_dict["pc_segment"] = seg[chosen]
        g = torch.Generator(device=coord.device)
        g.manual_seed(int(params.get("seed", 0)))
        idx = params.get("idx")
        if idx is not None:
            idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).to(coord.device)
        out = gt.grid_sample_train(coord, self.grid_size, generator=g, return_inverse=self.return_inverse,
                                   sampled_index=data_dict.get("sampled_index"), idx_unique=idx)
        idx32 = out["idx_unique"].to(torch.int32).contiguous()
        if "sampled_index" in out:
            data_dict["sampled_index"] = out["sampled_index"]
        if self.return_inverse:
            data_dict["inverse"] = out["inverse"]
        if self.return_grid_coord:
            data_dict["grid_coord"] = out["grid_coord"]
        for k in self.keys:
            if k in data_dict:
                data_dict[k] = gt.take_rows(data_dict[k], idx32)
        return data_dict


@TRANSFORMS.register_module()
class SphereCrop(Transform):
    """transform.py:1419-1548 over gpu_transforms.sphere_crop; params["center_index"] replays a recorded centre."""

    def __init__(self, point_max=80000, sample_rate=None, mode="random"):
        assert mode in ["random", "center", "all"]
        self.point_max, self.sample_rate, self.mode = point_max, sample_rate, mode

    def draw(self, rng, data_dict):
        return dict(u=float(rng.random()))

    def apply(self, data_dict, params):
        ci = params.get("center_index")
        if ci is None and self.mode == "random":
            ci = min(int(params["u"] * data_dict["coord"].shape[0]), data_dict["coord"].shape[0] - 1)
        return gt.sphere_crop(data_dict, self.point_max, self.sample_rate, self.mode, center_index=ci)


@TRANSFORMS.register_module()
class Collect(Transform):
    """transform.py:319-352 over gpu_transforms.collect"""

    def __init__(self, keys, offset_keys_dict=None, **kwargs):
        self.keys, self.offset_keys, self.kwargs = keys, offset_keys_dict, kwargs

    def apply(self, data_dict, params):
        return gt.collect(data_dict, self.keys, self.offset_keys, **self.kwargs)


class Compose:
    """The reference's Compose (transform.py:1667-1677) with a seedable host Generator for every draw and, with fuse=True, runs of
    rigid ops and of colour ops folded into one kernel pass each (module docstring).  `params` replays one recorded dict per op."""

    def __init__(self, cfg=None, fuse=True, seed=None):
        self.cfg = cfg if cfg is not None else []
        self.transforms = [TRANSFORMS.build(c) if isinstance(c, dict) else c for c in self.cfg]
        self.fuse = fuse
        self.rng = np.random.default_rng(seed)

    def __call__(self, data_dict, params=None):
        if params is not None and len(params) != len(self.transforms):
            raise ValueError("Compose: one params dict per transform")
        state = None
        for i, t in enumerate(self.transforms):
            p = params[i] if params is not None else t.draw(self.rng, data_dict)
            fam = t.family if self.fuse else None
            if state is not None and state.family != fam:
                state.flush(data_dict)
                state = None
            if fam is None:
                data_dict = t.apply(data_dict, p)
            else:
                if state is None:
                    state = _STATES[fam]()
                t.fold(state, data_dict, p)
        if state is not None:
            state.flush(data_dict)
        return data_dict
