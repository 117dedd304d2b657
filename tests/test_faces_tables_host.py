"""Host-only check of ops._per_faces, the "table built once per faces tensor" helper behind _vertex_face_csr, mesh_topology_of and
point_mesh_tables_of: the entry is keyed by the tensor's address, so it has to keep the tensor itself."""
import torch


def test_a_table_is_built_once_per_faces_tensor_and_keeps_it():
    from hifihr_amd import ops
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    built = []

    def build():
        built.append(len(built))
        return ["table", len(built)]

    before = set(ops._FACES_TABLES)
    try:
        first = ops._per_faces("test", faces, 4, build)
        assert ops._per_faces("test", faces, 4, build) is first and built == [0]
        table, kept = ops._FACES_TABLES[("test", faces.data_ptr(), 2, 4, "cpu")]
        assert table is first and kept is faces
        assert ops._per_faces("test", faces, 5, build) is not first and built == [0, 1]           # another vertex count: another table
        assert ops._per_faces("other", faces, 4, build) is not first and built == [0, 1, 2]       # another kind of table
        same_values = faces.clone()
        assert ops._per_faces("test", same_values, 4, build) is not first and len(built) == 4     # another tensor: its own entry
    finally:
        for key in set(ops._FACES_TABLES) - before:
            del ops._FACES_TABLES[key]


def test_vertex_face_csr_goes_through_it():
    from hifihr_amd import ops
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    off, idx = ops._vertex_face_csr(faces, 4)
    assert off.tolist() == [0, 2, 3, 5, 6] and idx.tolist() == [0, 4, 1, 2, 5, 6]         # (face * 4 + corner), vertex by vertex
    again = ops._vertex_face_csr(faces, 4)
    assert again[0] is off and again[1] is idx
    key = ("vertex_face_csr", faces.data_ptr(), 2, 4, "cpu")
    assert ops._FACES_TABLES[key][1] is faces
    del ops._FACES_TABLES[key]
