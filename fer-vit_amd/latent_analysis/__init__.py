"""Latent-space analysis (reference `latent_analysis/`): expression directions fitted on the device."""
