"""srcgan_amd -- MI355X (gfx950) native training hot path of huster-wgm/SRCGAN.

Exports the reference's names for the path (``from model import *`` at trainCas.py:12 resolves
``RDDBNet``; train.py:11 imports ``RDDBNetA, RDDBNetB, NLayerDiscriminator``; ``losses.L1Loss``, ``losses.DSSIMLoss``, ``losses.VGG16Loss``, ``losses.NearestSelector`` etc.).
Everything computes in libsrcgan_amd.so (hand-written HIP for gfx950); there is no CPU fallback.
"""
from ._native import set_default_dtype, LIB_PATH
from .model import RDDBNet, RDDBNetA, RDDBNetB, LegacyRDDBNet, ResDeconv, ESPCN, SRCNN, EDSR, SRDN, SRDenseNetA, SRDenseNetB, RCAN, DDBPN, RDN, MDSR, VDSR, NLayerDiscriminator, ResidualDenseBlock_5, RRDB
from .model import ResnetGenerator, UnetGenerator, define_G, get_norm_layer, init_weights, init_net
from .losses import (L1Loss, MSELoss, PSNRLoss, GANLoss, DSSIMLoss, VGG16Loss, PerceptionLoss, NearestSelector, NearestL1Loss,
                     L1Loss3D, DSSIMLoss3D, VGG16Loss3D, FLoss, CELoss, ConLoss, CrossLoss)
from .infer import plan_tiles, receptive_halo, upscale_scene, cascade_scene
from .metrics import score_scene

__all__ = ["RDDBNet", "RDDBNetA", "RDDBNetB", "LegacyRDDBNet", "ResDeconv", "ESPCN", "SRCNN", "EDSR", "SRDN", "SRDenseNetA", "SRDenseNetB", "RCAN", "DDBPN", "RDN", "MDSR", "VDSR", "ResnetGenerator", "UnetGenerator", "define_G", "get_norm_layer", "init_weights", "init_net", "NLayerDiscriminator", "ResidualDenseBlock_5", "RRDB",
           "L1Loss", "MSELoss", "PSNRLoss", "GANLoss", "DSSIMLoss", "VGG16Loss", "PerceptionLoss", "NearestSelector", "NearestL1Loss", "L1Loss3D", "DSSIMLoss3D", "VGG16Loss3D", "FLoss", "CELoss", "ConLoss", "CrossLoss", "plan_tiles", "receptive_halo", "upscale_scene", "cascade_scene", "score_scene", "set_default_dtype", "LIB_PATH"]
__version__ = "0.1.0"
