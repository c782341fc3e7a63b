"""Counterpart of the parts of the reference's lib/utils/preprocess.py that run/fitting.py and run/demo_fit.py use: ``compute_bbox``
(:136-159), ``bbox_from_detector`` (:117-134), ``load_obj`` (:23-31) and ``load_ply`` (:34-40, on a PLY reader of its own: ``plyfile`` is
not a dependency).  ``process_image`` / ``crop`` are not mirrored: they need cv2's resampler and produce ``norm_img`` / ``crop_ul`` /
``crop_br``, inputs of CLIFF's image network, which neither script reads."""
import numpy as np
import torch

from ..body_model import constants


def load_obj(file_name):
    """[V, 3] fp64: the coordinates of the ``v x y z`` records of a Wavefront OBJ file, in file order (fields separated by single
    blanks, as the reference reads them; ``vn`` / ``vt`` / ``f`` records are passed over)."""
    with open(file_name) as f:
        records = (line.split(" ") for line in f)
        rows = [[float(w) for w in rec[1:4]] for rec in records if rec[0] == "v"]
    return np.stack([np.array(r) for r in rows])


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(f, file_name):
    """(format, elements) with elements = [(name, count, [(property name, scalar type) or (property name, count type, item type)])]."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{file_name}: not a PLY file (no 'ply' magic line)")
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError(f"{file_name}: PLY header has no end_header line")
        words = raw.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        try:
            if words[0] == "end_header":
                break
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                elements.append((words[1], int(words[2]), []))
            elif words[0] == "property":
                if words[1] == "list":
                    elements[-1][2].append((words[4], _PLY_TYPES[words[2]], _PLY_TYPES[words[3]]))
                else:
                    elements[-1][2].append((words[2], _PLY_TYPES[words[1]]))
            else:
                raise KeyError(words[0])
        except (IndexError, KeyError, ValueError) as e:
            raise ValueError(f"{file_name}: malformed PLY header line {raw!r}") from e
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{file_name}: unsupported PLY format {fmt!r}")
    return fmt, elements


def load_ply(file_name):
    """[V, 3]: the ``x``, ``y``, ``z`` properties of the ``vertex`` element (in their common numpy type, as np.stack gives the reference).
    Reads ascii, binary_little_endian and binary_big_endian files; other properties, list properties and other elements are skipped by
    their declared sizes.  A malformed or truncated file raises ValueError naming the file."""
    with open(file_name, "rb") as f:
        fmt, elements = _ply_header(f, file_name)
        order = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
        for name, count, props in elements:
            is_vertex = name == "vertex"
            scalar = all(len(p) == 2 for p in props)
            if is_vertex:
                names = [p[0] for p in props]
                if not scalar or any(c not in names for c in "xyz"):
                    raise ValueError(f"{file_name}: the vertex element needs scalar x, y, z properties")
            try:
                if order is None:
                    rows = []
                    for _ in range(count):
                        line = f.readline()
                        if not line:
                            raise ValueError(f"{file_name}: truncated PLY body (element {name})")
                        if is_vertex:
                            words = line.split()
                            if len(words) < len(props):
                                raise ValueError(f"{file_name}: short vertex line {line!r}")
                            rows.append(words[:len(props)])
                    if is_vertex:
                        try:
                            cols = {p[0]: np.array([float(r[i]) for r in rows]).astype(np.dtype(p[1])) for i, p in enumerate(props) if p[0] in ("x", "y", "z")}
                        except ValueError as e:
                            raise ValueError(f"{file_name}: malformed vertex line in the PLY body") from e
                        return np.stack((cols["x"], cols["y"], cols["z"]), 1)
                elif scalar:
                    dt = np.dtype([(p[0], order + p[1]) for p in props])
                    buf = f.read(dt.itemsize * count)
                    if len(buf) != dt.itemsize * count:
                        raise ValueError(f"{file_name}: truncated PLY body (element {name})")
                    if is_vertex:
                        rec = np.frombuffer(buf, dtype=dt)
                        return np.stack(tuple(rec[c].astype(rec[c].dtype.newbyteorder("=")) for c in "xyz"), 1)
                else:
                    for _ in range(count):
                        for p in props:
                            if len(p) == 2:
                                n = np.dtype(p[1]).itemsize
                            else:
                                cbuf = f.read(np.dtype(p[1]).itemsize)
                                if len(cbuf) != np.dtype(p[1]).itemsize:
                                    raise ValueError(f"{file_name}: truncated PLY body (element {name})")
                                n = int(np.frombuffer(cbuf, dtype=order + p[1])[0]) * np.dtype(p[2]).itemsize
                            if len(f.read(n)) != n:
                                raise ValueError(f"{file_name}: truncated PLY body (element {name})")
            except (TypeError, OverflowError) as e:
                raise ValueError(f"{file_name}: malformed PLY body (element {name})") from e
    raise ValueError(f"{file_name}: PLY file has no vertex element")


def bbox_from_detector(bbox, rescale=1.1):
    """(centre, scale) of a detector box [min_x, min_y, max_x, max_y] (preprocess.py:117-134): the centre is the box's midpoint as a
    tensor, the scale the longer of (width x crop aspect ratio, height) over 200 pixels, widened by ``rescale``.  The operations and
    their order are the reference's (golden g29 holds its outputs bit for bit): sum then halve, difference, times ratio, / 200, x rescale."""
    lo, hi = (bbox[0], bbox[1]), (bbox[2], bbox[3])
    midpoint = torch.tensor([(lo[k] + hi[k]) / 2.0 for k in range(2)])
    width, height = hi[0] - lo[0], hi[1] - lo[1]
    return midpoint, max(width * constants.CROP_ASPECT_RATIO, height) / 200.0 * rescale


def compute_bbox(json_data):
    """[[person index, min_x, min_y, max_x, max_y]] over the visible (confidence > 0) OpenPose keypoints of every person of an OpenPose
    JSON record; a person with no visible keypoint is skipped (preprocess.py:136-159)."""
    bbox_list = []
    for batch_id, person in enumerate(json_data["people"]):
        keypoints = np.array(person["pose_keypoints_2d"]).reshape(-1, 3)
        visible = keypoints[keypoints[:, 2] > 0]
        if len(visible) == 0:
            continue
        bbox_list.append([batch_id, np.min(visible[:, 0]), np.min(visible[:, 1]), np.max(visible[:, 0]), np.max(visible[:, 1])])
    return np.array(bbox_list)
