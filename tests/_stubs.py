"""Collections over stand-in indexes for the CPU tests of the front end's host logic: built
through Collection's constructor (index=<stub>), never by setting its private fields. The
stand-in index classes stay with the tests, since they model different things."""


def stub_collection(index, dim=4, payloads=(), ids=None, tags=None, name="t"):
    """A Collection named `name` over `index` holding one point per payload: row r has id
    ids[r] (default r), payloads[r], version 1, and its tag coded into the collection's
    PayloadTags (`tags`: a filled codebook to use instead of a fresh one). The index itself is
    the caller's to fill."""
    from ragmi.collection import Collection
    col = Collection(name, dim, None, index=index)
    if tags is not None:
        col.tags = tags
    col.payloads = list(payloads)
    col.row_ids = list(range(len(col.payloads))) if ids is None else list(ids)
    col.id_to_row = {pid: r for r, pid in enumerate(col.row_ids)}
    for p in col.payloads:
        col.tags.tag(p)
    col.versions = [1] * len(col.payloads)
    col.op = 1 if col.payloads else 0
    return col


def stub_client(col):
    """A QdrantClient serving `col` under its name."""
    from ragmi.qdrant import QdrantClient
    client = QdrantClient()
    client._collections[col.name] = col
    return client, col
