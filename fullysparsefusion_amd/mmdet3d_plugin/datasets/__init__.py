from .pipelines import (Collect3D, DevicePointAssembler, Compose, DefaultFormatBundle3D, GlobalRotScaleTrans, LiDARPoints, LoadMaskFromFiles,  # noqa: F401
                        LoadPointsFromFile, LoadPointsFromMultiSweeps, MultiScaleFlipAug3D, MyLoadPointsFromFile,
                        MyLoadPointsFromMultiSweeps, NormalizePoints, PointsRangeFilter, RandomFlip3D, SaveNoAugPoints,
                        frame_to_device)
from .mask_paint import PaintMasksFromDetections  # noqa: F401,E402
from .train_augment import DeviceTrainAugment, draw_train_augmentation  # noqa: F401,E402
