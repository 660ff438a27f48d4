"""Data preparation (reference `data/`): latents pushed along verified non-expression directions."""
