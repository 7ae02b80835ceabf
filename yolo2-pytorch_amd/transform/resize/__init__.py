"""`transform.resize` — the resize plugins of config.ini (`[transform] resize_train` / `resize_eval`): transform.resize.label."""
