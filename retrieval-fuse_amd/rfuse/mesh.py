"""Mesh export of refined TSDF volumes: the last step of the reference's inference loop (trainer/train_refinement.py:170-173 ->
dataset/scene.py visualize_*_chunk -> util/visualization.py:34-37 ``visualize_sdf_as_mesh``: ``marching_cubes(sdf, 0.75)`` -> ``export_obj``).

PARITY UNPINNED: the reference calls the third-party ``marching_cubes`` package, which is neither in its tree nor pinned in requirements.txt.  What is
built is the marching-cubes construction itself -- one vertex per grid edge the level crosses (linear interpolation), per cube one closed polygon around
every group of "inside" (value < level) corners, fan-triangulated, oriented away from the inside -- on the device (csrc/mesh.hip), with the vertices
welded by grid edge.  Tested by invariants (vertices on crossed edges, closed oriented 2-manifold on closed shapes) and against the independent
restatement oracle/mesh.py; the triangulation inside a cube may differ from that package's table where a cube has several valid ones.

    verts, tris = marching_cubes(volume, 0.75)        # float32 [V, 3] in voxel-index coordinates, int32 [T, 3]
    visualize_sdf_as_mesh(volume, 'scene.obj')        # the reference's signature
"""
import numpy as np
import torch

from . import _lib
from .ops import _p, _stream, _device_scoped


def _corner(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edge_id(c0, c1):
    """cube edge between two corners that differ on one axis: axis * 4 + (u + 2 v), (u, v) = the corners' coordinates on the other two axes"""
    p0, p1 = _corner(c0), _corner(c1)
    (a,) = [i for i in range(3) if p0[i] != p1[i]]
    u, v = [p0[i] for i in range(3) if i != a]
    return a * 4 + u + 2 * v


def _faces():
    """the six faces as corner quadruples, counter-clockwise seen from outside the cube"""
    out = []
    for a in range(3):
        for side in (0, 1):
            u, v = [(1, 2), (2, 0), (0, 1)][a]
            if side == 0:
                u, v = v, u
            quad = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[u], p[v] = side, cu, cv
                quad.append(p[0] | p[1] << 1 | p[2] << 2)
            out.append(quad)
    return out


def build_tables():
    """-> (tri_table int8 [256, 16], tri_count int8 [256]).  Configuration bit c = corner c is inside.  On every face each maximal run of inside corners
    (walking the face counter-clockwise from outside) is cut off by one segment from the run's exit crossing to its entry crossing -- on a face with two
    diagonal inside corners that separates them, and since the rule reads nothing but the face's own four corners, the two cubes sharing a face agree:
    the surface is watertight.  Segments chain into closed loops (a crossing is an exit on one of its two faces and an entry on the other); loops in
    order of their smallest edge.  A loop is fan-triangulated, reversed so that normals point away from the inside, from the first of its vertices
    (starting at the smallest edge, in loop order) whose fan diagonals never join two cube edges of ONE face: on a face with four crossings such a
    diagonal would lie in the face plane, and the neighbouring cube -- which may draw the same one -- would make it an edge of four triangles.
    At most 5 triangles per cube."""
    faces = _faces()
    on_face = {}
    for e in range(12):
        a, u, v = e >> 2, e & 1, (e >> 1) & 1
        lo = [0, 0, 0]
        lo[[i for i in range(3) if i != a][0]], lo[[i for i in range(3) if i != a][1]] = u, v
        hi = list(lo)
        hi[a] = 1
        ends = {lo[0] | lo[1] << 1 | lo[2] << 2, hi[0] | hi[1] << 1 | hi[2] << 2}
        on_face[e] = {i for i, f in enumerate(faces) if ends <= set(f)}
    table = np.full((256, 16), -1, dtype=np.int8)
    count = np.zeros(256, dtype=np.int8)
    for cfg in range(256):
        nxt = {}
        for f in faces:
            ins = [(cfg >> c) & 1 for c in f]
            if sum(ins) in (0, 4):
                continue
            for k in range(4):
                if ins[k] and not ins[k - 1]:
                    j = k
                    while ins[(j + 1) % 4]:
                        j = (j + 1) % 4
                    nxt[_edge_id(f[j], f[(j + 1) % 4])] = _edge_id(f[k - 1], f[k])
        seen, tris = set(), []
        for e in sorted(nxt):
            if e in seen:
                continue
            loop, c = [e], nxt[e]
            seen.add(e)
            while c != e:
                loop.append(c)
                seen.add(c)
                c = nxt[c]
            for s in range(len(loop)):
                fan = loop[s:] + loop[:s]
                if all(not (on_face[fan[0]] & on_face[fan[i]]) for i in range(2, len(fan) - 1)):
                    break
            else:
                raise AssertionError('no admissible fan for configuration %d' % cfg)
            for i in range(1, len(fan) - 1):
                tris += [fan[0], fan[i + 1], fan[i]]
        assert len(tris) <= 15
        table[cfg, :len(tris)] = tris
        count[cfg] = len(tris) // 3
    return table, count


_TABLES = {}


def _device_tables(device):
    key = (device.type, device.index)
    if key not in _TABLES:
        table, count = build_tables()
        _TABLES[key] = (torch.from_numpy(table).to(device).contiguous(), torch.from_numpy(count).to(device).contiguous())
    return _TABLES[key]


@_device_scoped
@torch.no_grad()
def marching_cubes(volume, level=0.75):
    """volume: [X, Y, Z] float32 tensor on the GPU (or anything torch.as_tensor takes: it is moved to cuda:current).  -> (vertices float32 [V, 3] in
    voxel-index coordinates, triangles int32 [T, 3]) as device tensors; vertices in grid-edge order (x, y, z, axis), triangles in cube order."""
    v = torch.as_tensor(volume)
    if not v.is_cuda:
        v = v.to('cuda')
    v = v.to(torch.float32).contiguous()
    if v.dim() != 3 or min(v.shape) < 2:
        raise ValueError('marching_cubes: expected a [X, Y, Z] volume of at least 2^3 voxels, got %s' % (tuple(v.shape),))
    X, Y, Z = (int(s) for s in v.shape)
    lib = _lib.load()
    table, count = _device_tables(v.device)
    ntri = torch.empty(X * Y * Z, dtype=torch.int32, device=v.device)
    flag = torch.empty(X * Y * Z * 3, dtype=torch.int32, device=v.device)
    lib.rf_mc_classify(_p(v), X, Y, Z, float(level), _p(count), _p(ntri), _p(flag), _stream())
    tri_end, edge_end = torch.cumsum(ntri, 0, dtype=torch.int64), torch.cumsum(flag, 0, dtype=torch.int64)
    n_tri, n_vert = int(tri_end[-1].item()), int(edge_end[-1].item())            # the one host sync: output sizes
    tri_off, edge_off = (tri_end - ntri).contiguous(), (edge_end - flag).contiguous()
    verts = torch.empty((n_vert, 3), dtype=torch.float32, device=v.device)
    tris = torch.empty((n_tri, 3), dtype=torch.int32, device=v.device)
    if n_tri:
        lib.rf_mc_emit(_p(v), X, Y, Z, float(level), _p(table), _p(tri_off), _p(edge_off), _p(ntri), _p(flag), _p(verts), _p(tris), _stream())
    return verts, tris


def export_obj(vertices, triangles, path):
    """Wavefront .obj: 'v x y z' lines, then 'f a b c' with 1-based indices (what the reference's mc.export_obj writes)"""
    v = torch.as_tensor(vertices).detach().cpu().numpy().astype(np.float64)
    t = torch.as_tensor(triangles).detach().cpu().numpy().astype(np.int64) + 1
    with open(path, 'w') as f:
        if len(v):
            f.write('\n'.join('v %f %f %f' % (a, b, c) for a, b, c in v))
            f.write('\n')
        if len(t):
            f.write('\n'.join('f %d %d %d' % (a, b, c) for a, b, c in t))
            f.write('\n')


def load_obj(path):
    """Wavefront .obj -> (vertices float32 [V, 3], triangles int32 [T, 3], 0-based) as numpy arrays: the reader the mesh metrics need
    (rfuse/mesh_metrics.py compute_metrics; the reference goes through trimesh.load_mesh).  Reads 'v x y z [w]' and 'f ...' lines; a face index may
    be 'a', 'a/b', 'a//c' or 'a/b/c' (the vertex index is the first field), 1-based, negative = counted from the last vertex read so far; polygons
    are fan-triangulated from their first corner.  Every other line is ignored.  Round-trips ``export_obj`` (to the six decimals it writes)."""
    verts, tris = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == 'v':
                if len(parts) < 4:
                    raise ValueError('%s:%d: a vertex needs three coordinates' % (path, no))
                verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
            elif parts[0] == 'f':
                if len(parts) < 4:
                    raise ValueError('%s:%d: a face needs three corners' % (path, no))
                idx = [int(q.split('/')[0]) for q in parts[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                if 0 in [int(q.split('/')[0]) for q in parts[1:]]:
                    raise ValueError('%s:%d: face indices are 1-based' % (path, no))
                tris += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    v = np.array(verts, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    t = np.array(tris, dtype=np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError('%s: a face refers to vertex %d of %d' % (path, int(t.max() if t.max() >= len(v) else t.min()) + 1, len(v)))
    return v, t.astype(np.int32)


def visualize_sdf_as_mesh(sdf, output_path, level=0.75, scale_factor=1):
    """reference util/visualization.py:34-37, same arguments"""
    vertices, triangles = marching_cubes(sdf, level)
    export_obj(vertices / scale_factor, triangles, output_path)
