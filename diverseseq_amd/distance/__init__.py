"""Host side of the distance path.  It mirrors diverse_seq/distance.py (mash_sketches :178-227, mash_distances :119-175,
mash_distance :230-291, euclidean_distances :294-332) and the strided chunks of diverse_seq/cluster.py:607-644, with the
arithmetic in libdvs_hip.so, and adds the Jensen-Shannon divergence of k-mer frequencies as a third mode (jsd:
total_jsd of a two-member set, src/records.rs:27-68).  Everything behind the square matrix has no counterpart in the
reference.  An operation is defined once, as a method of `DeviceSide` -- what a mode keeps in HBM of one batch -- over
one C entry, which takes a `_lib.Source` (dvs_source: the mode and its handle, or a caller's matrix); the functions
over sequences, the matrix_* functions over a count matrix in HBM, the `Sketches` methods and cluster.py's functions
over a caller's own matrix are a few lines over it:

| DeviceSide         | over sequences                        | over a CountMatrix               | cluster.py, caller's matrix | C entry                | the distances      |
|--------------------|---------------------------------------|----------------------------------|-----------------------------|------------------------|--------------------|
| distances          | MODES[mode][0]: mash_distances, ...   | matrix_{euclidean,jsd}_distances | --                          | dvs_distances          | matrix held in HBM |
| linkage            | MODES[mode][1]: mash_linkage, ...     | --                               | linkage, average_linkage    | dvs_linkage            | matrix held in HBM |
| nj                 | NJ_MODES: mash_nj, ...                | --                               | neighbor_joining            | dvs_nj                 | matrix held in HBM |
| cross_distances    | cross_distances, CROSS_MODES[mode][0] | matrix_cross_distances           | --                          | dvs_cross_distances    | strip by strip     |
| nearest            | nearest, CROSS_MODES[mode][1]         | matrix_nearest                   | --                          | dvs_nearest            | strip by strip     |
| cluster_scores     | cluster_scores                        | matrix_cluster_scores            | cluster_scores              | dvs_cluster_scores     | strip by strip     |
| cophenet           | cophenet                              | matrix_cophenet                  | cophenet                    | dvs_cophenet           | strip by strip     |
| maxmin             | maxmin, MAXMIN_MODES                  | matrix_maxmin                    | maxmin                      | dvs_maxmin             | row per step       |
| within             | within, neighbours                    | matrix_within                    | within                      | dvs_within             | strip by strip     |
| threshold_clusters | threshold_clusters                    | matrix_threshold_clusters        | threshold_clusters          | dvs_threshold_clusters | strip by strip     |
| pcoa               | pcoa, PCOA_MODES                      | matrix_pcoa                      | pcoa                        | dvs_pcoa               | matrix held in HBM |
| pcoa_project       | pcoa_project                          | matrix_pcoa_project              | --                          | dvs_pcoa_project       | strip by strip     |
| kmedoids           | kmedoids, KMEDOIDS_MODES              | matrix_kmedoids                  | kmedoids                    | dvs_kmedoids           | matrix held in HBM |
| mst                | mst, MST_MODES                        | matrix_mst                       | minimum_spanning_tree       | dvs_mst                | strip by strip     |
| permanova          | permanova, PERMANOVA_MODES            | matrix_permanova                 | permanova                   | dvs_permanova          | matrix held in HBM |

The layers, each over those before it: `_results` (result types, limits, argument checks), `_calls` (`make_source`
and one `run_<op>` per C entry), `_sides` (`Sketches`, `DeviceSide`, `device_side`), `_sequences` (the public
functions).  This module is their public names."""

from __future__ import annotations

# what was reachable as an attribute of the single module this package replaced, beside its own names
import ctypes as C  # noqa: F401
from typing import NamedTuple  # noqa: F401

import numpy as np  # noqa: F401

from .. import engine  # noqa: F401
# the `__all__` of each layer
from ._results import *  # noqa: F401,F403
from ._calls import *  # noqa: F401,F403
from ._sides import *  # noqa: F401,F403
from ._sequences import *  # noqa: F401,F403
