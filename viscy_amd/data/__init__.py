from .hcs import HCSDataModule, SlidingWindowDataset  # noqa: F401
from .ome_zarr import open_ome_zarr, write_hcs_plate  # noqa: F401
from .combined import (BatchedConcatDataModule, CombinedDataModule, CombinedLoader, CombineMode, ConcatDataModule,  # noqa: F401
                       ShardedDistributedSampler)
from .triplet import FrameCache, TripletDataModule, TripletDataset  # noqa: F401
from .multi_experiment import (ChannelDropout, ExperimentRegistry, FlexibleBatchSampler, MultiExperimentDataModule,  # noqa: F401
                               MultiExperimentIndex, MultiExperimentTripletDataset, nearest_exact_index, parse_channel_name,
                               sample_tau)
