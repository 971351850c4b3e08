"""vulkan_radix_sort_amd -- MI355X (gfx950) HIP backend behind the VrdxSorter / vrdxCmdSort* API.

The product is the C-ABI shared library ``libvrdx_hip.so`` (sources in ``csrc/``, public header
``include/vk_radix_sort.h``).  This package is the thin Python host-side mirror of that interface
used by the tests and by ``bench.py``: same names, same argument meaning, same error behaviour as
the reference's ``include/vk_radix_sort.h`` (see :mod:`vulkan_radix_sort_amd.api`).

There is no CPU fallback: importing :mod:`vulkan_radix_sort_amd.api` raises if the HIP library has
not been built (``make -C vulkan_radix_sort_amd/csrc`` or ``__graft_entry__.build()``).
"""
from .api import (  # noqa: F401
    VK_SUCCESS,
    VrdxError,
    VrdxSorterStorageRequirements,
    Sorter,
    QueryPool,
    library_path,
    load_library,
    EXPORTED_SYMBOLS,
    version_string,
    event_overhead_ns,
    VrdxHipPlanInfo,
    PLAN_NAMES,
    STATUS_LOOKBACK_GAVE_UP,
    STATUS_RANK_ORDER,
    STATUS_SEGMENTS_INVALID,
    STATUS_COUNT_CLAMPED,
    STATUS_ENQUEUE_REFUSED,
    VERDICT_NONE,
    VERDICT_HYBRID8_RUNS,
    VERDICT_HYBRID8_DECLINED,
    VERDICT_MSD_RUNS,
    VERDICT_MSD_SORTED,
    KEY_UINT64,
    KEY_INT64,
    KEY_FLOAT64,
    ORDER_DESCENDING,
    KEY_ORDERS,
    order_word,
    KEY32_UINT32,
    KEY32_INT32,
    KEY32_FLOAT32,
    KEY32_ORDERS,
    order_word32,
    VrdxHipWideValuePlanInfo,
    WIDE_VALUE_FORM_NAMES,
    WIDE_VALUE_SEGMENTED_CALLS,
    VrdxHipRangeSortPlanInfo,
    RANGE_SORT_FORM_NAMES,
    RANGE_SORT_CALLS,
    VrdxHipBalancedSegmentedPlanInfo,
    VrdxHipBalancedSplitInfo,
    BALANCED_FORM_NAMES,
    BALANCED_SEGMENTED_CALLS,
    BALANCED_EXPORTED_SYMBOLS,
)
from .segmented import sort_segments  # noqa: F401
from .sort64 import sort64  # noqa: F401
from .segmented64 import sort_segments64  # noqa: F401
from .sort_bits import sort_bits  # noqa: F401
from .segmented_bits import sort_segments_bits  # noqa: F401
from .ordered import sort_ordered, sort_segments_ordered  # noqa: F401
from .wide_value import sort_key_value64, sort_segments_key_value64  # noqa: F401
from .range_sort import sort_range  # noqa: F401
from .segmented_balanced import sort_segments_balanced  # noqa: F401

__all__ = [
    "VK_SUCCESS",
    "VrdxError",
    "VrdxSorterStorageRequirements",
    "Sorter",
    "QueryPool",
    "library_path",
    "load_library",
    "EXPORTED_SYMBOLS",
    "version_string",
    "event_overhead_ns",
    "VrdxHipPlanInfo",
    "PLAN_NAMES",
    "STATUS_LOOKBACK_GAVE_UP",
    "STATUS_RANK_ORDER",
    "STATUS_SEGMENTS_INVALID",
    "STATUS_COUNT_CLAMPED",
    "STATUS_ENQUEUE_REFUSED",
    "VERDICT_NONE",
    "VERDICT_HYBRID8_RUNS",
    "VERDICT_HYBRID8_DECLINED",
    "VERDICT_MSD_RUNS",
    "VERDICT_MSD_SORTED",
    "KEY_UINT64",
    "KEY_INT64",
    "KEY_FLOAT64",
    "ORDER_DESCENDING",
    "KEY_ORDERS",
    "order_word",
    "sort_segments",
    "sort64",
    "sort_segments64",
    "sort_bits",
    "sort_segments_bits",
    "KEY32_UINT32",
    "KEY32_INT32",
    "KEY32_FLOAT32",
    "KEY32_ORDERS",
    "order_word32",
    "sort_ordered",
    "sort_segments_ordered",
    "VrdxHipWideValuePlanInfo",
    "WIDE_VALUE_FORM_NAMES",
    "sort_key_value64",
    "sort_segments_key_value64",
    "WIDE_VALUE_SEGMENTED_CALLS",
    "VrdxHipRangeSortPlanInfo",
    "RANGE_SORT_FORM_NAMES",
    "RANGE_SORT_CALLS",
    "sort_range",
    "VrdxHipBalancedSegmentedPlanInfo",
    "VrdxHipBalancedSplitInfo",
    "BALANCED_FORM_NAMES",
    "BALANCED_SEGMENTED_CALLS",
    "BALANCED_EXPORTED_SYMBOLS",
    "sort_segments_balanced",
]
