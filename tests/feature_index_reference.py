"""The numpy statement of the feature index (freud_amd/feature_index.py, freud_amd/csrc/findex.h) and of its queries on dense
series.  Shared by the CPU and the GPU tests; nothing here imports the code under test except write_reference_index, which hands
the reference lists to the project's own file writer so that the reader can be tested without a GPU."""
import numpy as np

TIMESTEP_S = 30 / 1500


def reference_index(values, indices, n_dict, pos0=0):
    """values / indices [rows, K] (any leading shape is flattened to rows) -> starts int64 [n_dict + 1], positions uint32 [nnz],
    value bits uint32 [nnz], stats dict.  Flatten, mask v != 0 and the index range, stable argsort by latent."""
    K = values.shape[-1]
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    i = np.asarray(indices).reshape(-1).astype(np.int64)
    bits = v.view(np.uint32)
    row = np.arange(v.size, dtype=np.int64) // K
    nonzero = (bits & np.uint32(0x7FFFFFFF)) != 0
    inside = (i >= 0) & (i < n_dict)
    keep = nonzero & inside
    order = np.argsort(i[keep], kind="stable")
    positions = (row[keep][order] + int(pos0)).astype(np.uint32)
    vbits = bits[keep][order]
    starts = np.zeros(n_dict + 1, np.int64)
    np.cumsum(np.bincount(i[keep], minlength=n_dict), out=starts[1:])
    stats = {"slots": int(v.size), "zero_slots": int((~nonzero).sum()), "out_of_range": int((nonzero & ~inside).sum()),
             "posted": int(keep.sum())}
    return starts, positions, vbits, stats


def verify_count(starts, positions, limit):
    """Slots whose position is not strictly greater than its predecessor's in the same list, or is >= limit."""
    p = positions.astype(np.int64)
    bad = p >= int(limit)
    if p.size > 1:
        same_list = np.ones(p.size, bool)
        same_list[starts[:-1][starts[:-1] < p.size]] = False          # the first slot of a list has no predecessor
        bad[1:] |= same_list[1:] & (p[1:] <= p[:-1])
    return int(bad.sum())


def dense_series(values, indices, n_dict):
    """[F, T, K] store -> float32 [n_dict, F, T] by the reference's rule (one matching slot per row)."""
    F, T, K = values.shape
    out = np.zeros((n_dict, F, T), np.float32)
    for q in range(K):
        j = np.asarray(indices[:, :, q], dtype=np.int64)
        ok = (j >= 0) & (j < n_dict)
        f, t = np.nonzero(ok)
        out[j[ok], f, t] += values[:, :, q][ok]
    return out


def top_activations_dense(series, filenames, n_files, max_val=None, min_val=None, absolute_magnitude=False, lengths=None):
    """The reference's top_activations (src/utils/activations.py:61-132) on a dense float32 [F, T] series of one latent:
    (pq, max_per_file), pq entries (filename, trimmed series, value, time)."""
    pq, mpf = [], []
    for f in range(series.shape[0]):
        a = series[f, : series.shape[1] if lengths is None else min(int(lengths[f]), series.shape[1])]
        if absolute_magnitude:
            signed = float(a[int(np.argmax(np.abs(a)))])
            value = abs(signed)
        else:
            signed = value = float(a.max())
        mpf.append(signed)
        if (max_val is not None and signed > max_val) or (min_val is not None and signed < min_val):
            continue
        pq.append((filenames[f], a, value, int(np.argmax(a)) * TIMESTEP_S))
        pq.sort(key=lambda e: e[2], reverse=True)
        pq = pq[:n_files]
    return pq, mpf


def write_reference_index(folder, layer_name, n_files=None, overwrite=False):
    """The index files of the store in `folder`, from reference_index through the project's writer (no GPU)."""
    from freud_amd import feature_index as fi
    from freud_amd.collect_features import FeatureShards
    sh = FeatureShards(folder, layer_name)
    n_files = len(sh) if n_files is None else n_files
    v = np.asarray(sh.values[:n_files]).reshape(n_files * sh.T, sh.K)
    i = np.asarray(sh.indices[:n_files]).reshape(n_files * sh.T, sh.K)
    starts, positions, vbits, stats = reference_index(v, i, sh.n_dict)
    w = fi.IndexWriter(folder, layer_name, overwrite)
    w.open(starts)
    w.write(0, positions, vbits.view(np.float32))
    meta = fi.index_metadata(n_files, sh.T, sh.K, sh.n_dict, str(sh.indices.dtype), starts, stats, 1,
                             fi.store_fingerprint(folder, layer_name, sh.filenames[:n_files]))
    w.finish(meta)
    return starts, positions, vbits, stats
