"""`transform` — the package of the transform plugins that config.ini names in `[transform]` (`transform.augmentation.RandomFlipHorizontally`,
`transform.resize.label.RandomCrop`, ...); `utils.parse_attr` resolves the dotted names.

Only the transforms whose pixel work the collate kernel does are here.  They do the reference's label arithmetic and RECORD the geometry
(`data['window']`, `data['flip']`) instead of resampling `data['image']`; utils.data has the rest of the collate step."""
