"""Drop-in stand-in for the reference's ``style_transfer`` package (train_style_transfer_nnfm.py imports
``style_transfer.fx.VGG16FeatureExtractor``), backed by the HIP convolutions of trase_amd.vgg."""
